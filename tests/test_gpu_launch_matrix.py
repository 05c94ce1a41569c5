"""GPU: the per-launch bound of tests/test_gpu_layers.py (every element of every launch against
the reference of the same operation fed with the GPU's own input blob, tests/launch_check.py) at
the kernel instantiations, tile branches and shape edges the bench geometry does not reach.

Each case first asserts from the launch log that the instantiation it exists for actually ran (a
planner change cannot silently empty it), then runs the checker on frames {first, last}; biases are
random and non-zero, PReLU slopes in (0.05, 0.5) (launch_check.random_params).  The tile branch is
chosen from tiles = frames (H + 2B)(W + 2B) / 256 x n-blocks (conv3_shape, conv3.hip): >= 768 the
16-wave / persistent 512-position tiles, >= 512 two 256-position tiles per CU, else one.

  a  c1 3->64 ReLU, c2 64->64 PReLU, pool, c3 64->128, 1x1 head at 4 x 184 x 328 (959 tiles, four
     even 82-column strips), CONV1_FUSED=0: fp16 conv3w8_kernel<64,1,1> (pooled epilogue)
  b  the same with POOL_FUSE=0: fp16 conv3w8_kernel<64,1,0>; pool1 and net_output bit-identical
     to (a), and, with conv1_2's blob, to CONV3W8_64=0 (conv3_kernel's 256 x 64 tiles)
  c  the same graph at 4 x 183 x 327, default switches: odd sizes turn conv1 fusion and pool fusion
     off themselves; strips of 82, 82, 82, 81 columns; ceil pooling in the stand-alone pool
  d  c1 3->64, c2 64->64, c3 64->128, c4 128->96, 1x1 head at 48 x 254 x 14 (VW = 16, exactly 768
     tiles), both precisions: the strip is too narrow for the persistent kernels -- c2 on the
     8-wave 256 x 64 tiles (the forward used to throw "conv3w8<64>: unsupported conv"), c3 / c4 on
     the 16-wave conv3_kernel over the strip geometry chosen for the persistent kernel
  e  the graph of test_conv3_tile_variants_bit_identical at 2 x 256 x 386 (persistent strips: four
     of 78 columns and one of 74): conv3w, conv3w8<128,2> and <128,4>; and with CONV3_W16=0,
     CONV1_TILE=0 the 8-wave 256-position tiles
  f  BODY_25 at 2 x 64 x 96 and 1 x 50 x 90 (odd at every level after the pools), both precisions
  g  the 7x7 CPM stages (3-pixel border) at 2 x 64 x 96, both precisions (the planner runs 7x7 in
     split precision on conv3_kernel's split instantiations)
  h  BODY_25 at the multi-scale sizes 1 x 80 x 160, 1 x 176 x 320 and 1 x 272 x 480, both
     precisions; split also against the fp32 oracle of the whole net
"""
import contextlib
import os
import tempfile
import time

import numpy as np
import pytest
import torch

from oracle import body25
from openpose_amd.api import PRECISION_SPLIT, Net, dev_switches
from tests import prototxt
from tests.launch_check import check_launches, conv_instantiations, print_rows, random_params
from tests.test_gpu_net import (SPLIT_CHANNEL_TOL, SPLIT_TOL, channel_errors, conv, cpm_stage_graph,
                                rel_l2)

pytestmark = pytest.mark.gpu

PERSISTENT = ("conv3w8_kernel", "conv3w_kernel", "conv3p_kernel")


@contextlib.contextmanager
def forwarded(ctx, model, params, x, split=False, **switches):
    """A net of `model` (a layer list or "builtin:...") after one forward of x under LAUNCH_LOG=1
    and the given dev switches; yields (net, launch log) and closes the net."""
    path = None
    if not isinstance(model, str):
        with tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False) as f:
            f.write(prototxt.emit(model))
            path = f.name
    net = None
    try:
        with dev_switches(LAUNCH_LOG=1, **switches):
            net = Net(ctx, path or model)
            net.set_params(params)
            if split:
                net.set_precision(PRECISION_SPLIT)
            net.forward(torch.from_numpy(x).cuda())
            log = net.launch_log()
        yield net, log
    finally:
        if net is not None:
            net.close()
        if path:
            os.unlink(path)


def image(seed, shape):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, shape).astype(np.float32)


def report(record_property, title, rows):
    print_rows(rows, title)
    worst = max(r.frac for r in rows)
    record_property("max_frac_of_bound", round(worst, 4))
    return worst


def ran(log, prefix, split=None):
    return any(k.startswith(prefix) and (split is None or k.endswith(",split>") == split)
               for _, k in log)


def every_conv_once(log, graph):
    """Every conv of the graph is in exactly one launch-log layer (frame runs repeat a layer)."""
    layers = list(dict.fromkeys(layer for layer, _ in log if layer != "pool"))
    named = [c for layer in layers for c in layer.split("+") if c != "pool"]
    assert sorted(named) == sorted(l["name"] for l in graph if l["type"] == "Convolution")


# ---- a, b, c: the fp16 64-output tile of conv3w8 ------------------------------------------------

def front_graph():
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", 64, 3, "prelu")
    L.append(dict(name="pool1", type="Pooling", bottom=["c2"], top=["pool1"], kernel_size=2, stride=2))
    L += conv("c3", "pool1", 128, 3, "prelu") + conv("c4", "c3", 52, 1)
    L.append(dict(name="net_output", type="Concat", bottom=["c4"], top=["net_output"]))
    return L


AB_SWITCHES = {"a": dict(CONV1_FUSED=0), "b": dict(CONV1_FUSED=0, POOL_FUSE=0),
               "w8_64_off": dict(CONV1_FUSED=0, POOL_FUSE=0, CONV3W8_64=0)}
AB_KERNEL = {"a": "conv3w8_kernel<64,1,1,", "b": "conv3w8_kernel<64,1,0,", "w8_64_off": "conv3_kernel<256,64,"}
_AB = {}


def ab_run(ctx, name):
    """One variant of cases (a) / (b) at 4 x 184 x 328, run and checked once per session: its log,
    checker rows and the blobs the variants must agree on."""
    if name not in _AB:
        L = front_graph()
        graph = prototxt.parse(prototxt.emit(L))
        params = random_params(graph, 81)
        x = image(82, (4, 3, 184, 328))
        with forwarded(ctx, L, params, x, **AB_SWITCHES[name]) as (net, log):
            blobs = {"pool1": net.blob("pool1"), "net_output": net.output_numpy()}
            if "POOL_FUSE" in AB_SWITCHES[name]:
                blobs["c2"] = net.blob("c2")
            k = conv_instantiations(log, ["c2"])["c2"]
            assert len(k) == 1 and k[0].startswith(AB_KERNEL[name]) and "split" not in k[0], log
            _AB[name] = dict(log=log, blobs=blobs)
            _AB[name]["rows"] = check_launches(net, graph, params, x, [0, 3], log=log)
    assert "rows" in _AB[name], "the per-launch check of this variant failed in an earlier test"
    return _AB[name]


def test_a_fp16_conv3w8_64_pooled(ctx, record_property):
    r = ab_run(ctx, "a")   # (asserts conv3w8_kernel<64,1,1 ran, then checks every launch)
    assert [layer for layer, _ in r["log"] if layer.startswith("c2")] == ["c2+pool"]
    report(record_property, "a: 4x184x328 CONV1_FUSED=0", r["rows"])


def test_b_fp16_conv3w8_64_unpooled(ctx, record_property):
    r = ab_run(ctx, "b")   # (asserts conv3w8_kernel<64,1,0 ran, then checks every launch)
    assert any(layer == "pool" for layer, _ in r["log"])
    report(record_property, "b: 4x184x328 CONV1_FUSED=0 POOL_FUSE=0", r["rows"])


def test_ab_variants_bit_identical(ctx, record_property):
    """pool1 and net_output are the same bits whether pool1 runs in conv3w8<64>'s epilogue or as
    its own kernel, and -- with conv1_2's own blob, materialised only without the pool fusion --
    whether the 64-output layer runs on conv3w8<64> or on conv3_kernel's 256 x 64 tiles."""
    a, b, off = ab_run(ctx, "a"), ab_run(ctx, "b"), ab_run(ctx, "w8_64_off")
    assert np.abs(a["blobs"]["pool1"]).max() > 0
    for name in ("pool1", "net_output"):
        np.testing.assert_array_equal(a["blobs"][name], b["blobs"][name], err_msg=name)
    for name in ("c2", "pool1", "net_output"):
        np.testing.assert_array_equal(b["blobs"][name], off["blobs"][name], err_msg=name)
    report(record_property, "CONV3W8_64=0 POOL_FUSE=0", off["rows"])


def test_c_fp16_conv3w8_64_odd_sizes(ctx, record_property):
    L = front_graph()
    graph = prototxt.parse(prototxt.emit(L))
    params = random_params(graph, 83)
    x = image(84, (4, 3, 183, 327))
    with forwarded(ctx, L, params, x) as (net, log):
        k = conv_instantiations(log, ["c1", "c2"])
        assert k["c1"][0].startswith("conv_image_kernel"), log     # no conv1 fusion at odd sizes
        assert k["c2"][0].startswith("conv3w8_kernel<64,1,0,"), log
        assert [layer for layer, _ in log].count("pool") == 1
        assert net.blob("pool1", (0, 1)).shape == (1, 64, 92, 164)   # ceil pooling
        rows = check_launches(net, graph, params, x, [0, 3], log=log)
    assert rows[-1].layer == "pool1"
    report(record_property, "c: 4x183x327", rows)


# ---- d: strips too narrow for the persistent kernels --------------------------------------------

@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
def test_d_narrow_strip_falls_back(ctx, record_property, split):
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", 64, 3, "prelu")
    L += conv("c3", "c2", 128, 3, "relu") + conv("c4", "c3", 96, 3, "prelu") + conv("c5", "c4", 52, 1)
    L.append(dict(name="net_output", type="Concat", bottom=["c5"], top=["net_output"]))
    graph = prototxt.parse(prototxt.emit(L))
    params = random_params(graph, 85)
    x = image(86, (48, 3, 254, 14))
    assert 48 * (254 + 2) * (14 + 2) // 256 == 768   # the 16-wave / persistent threshold
    with forwarded(ctx, L, params, x, split=split) as (net, log):
        k = conv_instantiations(log, ["c2", "c3", "c4"])
        for name, ks in k.items():
            assert len(ks) == 1 and not ks[0].startswith(PERSISTENT), (name, ks)
            assert ks[0].endswith(",split>") == split, (name, ks)
        # the 64-output layer on the 8-wave tiles it had before conv3w8's BN = 64 tile; the wider
        # ones on the 16-wave kernel, on the strip chosen for the persistent one
        assert k["c2"][0].startswith("conv3_kernel<256,64,448,"), k
        assert k["c3"][0].startswith("conv3_kernel<512,128,704,3,1,3,16"), k
        assert k["c4"][0].startswith("conv3_kernel<512,96,704,3,1,3,16"), k
        rows = check_launches(net, graph, params, x, [0, 47], split=split, log=log)
    report(record_property, "d: 48x254x14 %s" % ("split" if split else "fp16"), rows)


# ---- e: uneven persistent strips; the 8-wave 256-position tiles ---------------------------------

def variants_graph():
    """The graph of test_gpu_net.test_conv3_tile_variants_bit_identical."""
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", 128, 3, "relu")
    L += conv("c3", "c2", 96, 3, "prelu") + conv("c4", "c3", 128, 3, "prelu")
    L += conv("c5", "c4", 96, 3, "relu")
    L.append(dict(name="cat", type="Concat", bottom=["c3", "c5"], top=["cat"]))
    L += conv("c6", "cat", 128, 3, "prelu") + conv("c6b", "c6", 256, 3, "relu")
    L += conv("c6d", "c6b", 512, 3, "prelu")
    L += conv("c6c", "c6d", 512, 1, "prelu") + conv("c7", "c6c", 52, 1)
    L.append(dict(name="net_output", type="Concat", bottom=["c7"], top=["net_output"]))
    return L


@pytest.mark.parametrize("name,switches,must_run", [
    ("persistent", {}, ("conv3w_kernel<", "conv3w8_kernel<128,2", "conv3w8_kernel<128,4")),
    ("w8", {"CONV3_W16": 0, "CONV1_TILE": 0}, ("conv3_kernel<256,128,448,", "conv3_kernel<256,96,448,"))],
    ids=["persistent", "w8"])
def test_e_uneven_strips(ctx, record_property, name, switches, must_run):
    L = variants_graph()
    graph = prototxt.parse(prototxt.emit(L))
    params = random_params(graph, 87)
    x = image(88, (2, 3, 256, 386))
    with forwarded(ctx, L, params, x, **switches) as (net, log):
        for prefix in must_run:
            assert ran(log, prefix), (prefix, log)
        if switches:   # no 16-wave tile and no persistent kernel left
            assert not any(k.startswith(PERSISTENT) or (k.startswith("conv3_kernel") and k.endswith(",16>"))
                           for _, k in log), log
        rows = check_launches(net, graph, params, x, [0, 1], log=log)
    report(record_property, "e: 2x256x386 %s" % name, rows)


# ---- f, h: BODY_25 at small, odd and the multi-scale sizes --------------------------------------

def body25_case(ctx, record_property, title, shape, split, seed, whole_net=False):
    graph = body25.layers()
    params = random_params(graph, seed)
    x = image(seed + 1, shape)
    with forwarded(ctx, "builtin:BODY_25", params, x, split=split) as (net, log):
        every_conv_once(log, graph)
        convk = [k for _, k in log if k.startswith("conv")]
        assert all(("split" in k) == split for k in convk), convk
        t0 = time.time()
        rows = check_launches(net, graph, params, x, sorted({0, shape[0] - 1}), split=split, log=log)
        print("%s: references of %d launches in %.1f s" % (title, len(rows), time.time() - t0))
        got = net.output_numpy()
    report(record_property, title, rows)
    if whole_net:
        ref = body25.forward(x, params, graph=graph)
        err, ch = rel_l2(got, ref), channel_errors(got, ref).max()
        print("%s: rel-L2 %.3e, worst channel %.3e vs the fp32 oracle" % (title, err, ch))
        record_property("rel_l2", err)
        record_property("worst_channel", ch)
        assert err < SPLIT_TOL
        assert ch < SPLIT_CHANNEL_TOL


@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
@pytest.mark.parametrize("shape", [(2, 3, 64, 96), (1, 3, 50, 90)], ids=["2x64x96", "1x50x90"])
def test_f_body25_small_and_odd(ctx, record_property, shape, split):
    body25_case(ctx, record_property, "f: BODY_25 %dx%dx%d %s" % (shape[0], shape[2], shape[3],
                                                                 "split" if split else "fp16"),
                shape, split, 91)


@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
@pytest.mark.parametrize("hw", [(80, 160), (176, 320), (272, 480)], ids=["80x160", "176x320", "272x480"])
def test_h_body25_multi_scale_sizes(ctx, record_property, hw, split):
    """The smaller scales of a four-scale run at 656 x 368 (scale gap 0.25).  Split precision also
    against the fp32 oracle of the whole net, at the tolerances of test_gpu_net.py."""
    body25_case(ctx, record_property, "h: BODY_25 1x%dx%d %s" % (hw + ("split" if split else "fp16", )),
                (1, 3) + hw, split, 93, whole_net=split)


# ---- g: 7x7 kernels, 3-pixel border --------------------------------------------------------------

@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
def test_g_7x7_cpm_stages(ctx, record_property, split):
    L = cpm_stage_graph(True)
    graph = prototxt.parse(prototxt.emit(L))
    params = random_params(graph, 95)
    x = image(96, (2, 3, 64, 96))
    with forwarded(ctx, L, params, x, split=split) as (net, log):
        every_conv_once(log, graph)
        assert ran(log, "conv3_kernel<256,128,1024,", split), log
        assert ran(log, "conv3_kernel<256,96,1024,", split), log
        rows = check_launches(net, graph, params, x, [0, 1], split=split, log=log)
    report(record_property, "g: 7x7 CPM stages 2x64x96 %s" % ("split" if split else "fp16"), rows)
