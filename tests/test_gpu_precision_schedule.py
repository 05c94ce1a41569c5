"""GPU: nets under a per-layer precision schedule (Net.set_precision_schedule): every launch against
the reference of its own precision (tests/schedule_check.py), uniform schedules against
set_precision, re-planning, the hi-only kernels against the three-product kernels over a zero twin
(SPLIT_XHI=0), pools and the small-batch tiles.

  1  BODY_25 at 2 x 64 x 96 and 1 x 50 x 90 (test_gpu_launch_matrix case f) under three schedules --
     fp16 trunk + split stages, split trunk + fp16 stages, alternating by conv index: every kind of
     boundary, concats with fp16 and split members, fused and mixed head pairs
  2  uniform schedules: launch log and net_output of set_precision, bit for bit
  3  mixed -> forward -> uniform -> forward equals a fresh net of that precision, bit for bit
  4  the tile-variant graph of case e at 2 x 256 x 386 (persistent geometry; conv_kernels plans
     conv3w8 for every 3x3 layer there in split precision, so no other frame count is needed):
     first conv fp16, the rest split -- conv3w8x_kernel<128,1 ran, per-launch check, SPLIT_XHI=0
     equal values; two more schedules reach conv3w8x_kernel<96,1, <128,2 and <128,4; the same A/B
     on conv3_kernel's hi-only instantiations with BODY_25 at 2 x 64 x 96
  5  front_graph (c1, c2, pool, c3, 1x1 head) at 4 x 184 x 328, CONV1_FUSED=0: c2 split with c3 fp16
     and the reverse, POOL_FUSE 1 and 0 -- the pool exact, the variants bit-identical
  6  small-batch on against off under a mixed schedule at 1 x 64 x 96, bit-identical
  7  recorded with (1), not asserted: rel-L2 of each mixed net_output against the fp32 oracle,
     next to uniform fp16 and uniform split of the same run (record_property)
"""
import contextlib
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import body25
from openpose_amd.api import PRECISION_FP16, PRECISION_SPLIT, Net, dev_switches
from tests import prototxt
from tests.launch_check import conv_instantiations, print_rows, random_params
from tests.schedule_check import check_schedule
from tests.test_gpu_launch_matrix import every_conv_once, front_graph, image, variants_graph
from tests.test_gpu_net import rel_l2

pytestmark = pytest.mark.gpu

FP16, SPLIT = PRECISION_FP16, PRECISION_SPLIT


def trunk(c):
    return not c["name"].startswith("Mconv")


SCHEDULES = {
    "fp16_trunk": lambda c: FP16 if trunk(c) else SPLIT,
    "split_trunk": lambda c: SPLIT if trunk(c) else FP16,
    "alternating": lambda c: c["index"] % 2,
}


def hi_only(kernel):
    return kernel.endswith(",split,xhi>")


@contextlib.contextmanager
def scheduled(ctx, model, params, schedule=None, precision=None, small=False):
    """A net of `model` (a layer list or "builtin:...") with its weights set and the schedule (or
    the uniform precision) applied; yields the net and closes it."""
    path = None
    if not isinstance(model, str):
        with tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False) as f:
            f.write(prototxt.emit(model))
            path = f.name
    net = None
    try:
        net = Net(ctx, path or model)
        net.set_params(params)
        if small:
            net.set_small_batch(True)
        if precision is not None:
            net.set_precision(precision)
        if schedule is not None:
            net.set_precision_schedule(schedule)
        yield net
    finally:
        if net is not None:
            net.close()
        if path:
            os.unlink(path)


def forward(net, x):
    """(launch log, net_output) of one forward under LAUNCH_LOG=1.  (Dev switches that change the
    plan go around the net's whole life: a shape is planned once, at its first forward.)"""
    with dev_switches(LAUNCH_LOG=1):
        net.forward(torch.from_numpy(x).cuda())
        return net.launch_log(), net.output_numpy()


def named(net):
    return dict(zip([c["name"] for c in net.convs()], net.precision_schedule()))


def all_blobs(net, graph, frames=None):
    """Every materialised top of the graph (hi + lo), by name; frames: (first, count), default all."""
    out = {}
    for l in graph:
        if l["type"] not in ("Convolution", "Pooling", "Concat"):
            continue
        try:
            out[l["top"][0]] = net.blob(l["top"][0], frames)
        except Exception as e:
            assert "kept on chip" in str(e), e
    return out


def assert_equal_values(a, b):
    """Equal as values, element for element (the sign of a zero may differ)."""
    assert sorted(a) == sorted(b)
    for name in a:
        assert a[name].shape == b[name].shape and not np.isnan(a[name]).any(), name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)


@pytest.fixture(scope="module")
def body():
    graph = body25.layers()
    return graph, random_params(graph, 91)


_FP32 = {}


def fp32_reference(ctx, body, shape):
    """Once per shape: the image batch, the fp32 oracle's net_output and the rel-L2 of the two
    uniform precisions against it."""
    if shape not in _FP32:
        graph, params = body
        x = image(92, shape)
        ref = body25.forward(x, params, graph=graph)
        uniform = {}
        for name, prec in (("uniform_fp16", FP16), ("uniform_split", SPLIT)):
            with scheduled(ctx, "builtin:BODY_25", params, precision=prec) as net:
                uniform[name] = float(rel_l2(forward(net, x)[1], ref))
        _FP32[shape] = (x, ref, uniform)
    return _FP32[shape]


# ---- 1 (and 7): every boundary kind, per launch -------------------------------------------------

@pytest.mark.parametrize("name", sorted(SCHEDULES))
@pytest.mark.parametrize("shape", [(2, 3, 64, 96), (1, 3, 50, 90)], ids=["2x64x96", "1x50x90"])
def test_1_body25_mixed_per_launch(ctx, record_property, body, shape, name):
    graph, params = body
    x, ref, uniform = fp32_reference(ctx, body, shape)
    with scheduled(ctx, "builtin:BODY_25", params, SCHEDULES[name]) as net:
        log, out = forward(net, x)
        every_conv_once(log, graph)
        sched = named(net)
        # every launch runs in the precision of its convs, and the hi-only kernels took part
        for layer, k in log:
            if layer == "pool":
                continue
            split = {sched[c] for c in layer.split("+") if c != "pool"}
            assert len(split) == 1 and ("split" in k) == (split.pop() == SPLIT), (layer, k)
        # (a split trunk reads split blobs only: no boundary into split)
        assert any(hi_only(k) for _, k in log) == (name != "split_trunk"), log
        assert any(k.endswith(",split>") for _, k in log), log
        rows = check_schedule(net, graph, params, x, sorted({0, shape[0] - 1}), sched, log=log)
    print_rows(rows, "1: BODY_25 %dx%dx%d %s" % (shape[0], shape[2], shape[3], name))
    record_property("max_frac_of_bound", round(max(r.frac for r in rows), 4))
    # (7) recorded, not asserted
    rel = dict(uniform, **{name: float(rel_l2(out, ref))})
    print("7: rel-L2 vs the fp32 oracle: " + ", ".join("%s %.3e" % kv for kv in sorted(rel.items())))
    for k, v in rel.items():
        record_property("rel_l2_" + k, v)


# ---- 2: uniform schedules are set_precision -------------------------------------------------------

@pytest.mark.parametrize("prec", [FP16, SPLIT], ids=["fp16", "split"])
def test_2_uniform_schedule_equals_set_precision(ctx, body, prec):
    graph, params = body
    x = image(92, (2, 3, 64, 96))
    with scheduled(ctx, "builtin:BODY_25", params, precision=prec) as a:
        log_a, out_a = forward(a, x)
    with scheduled(ctx, "builtin:BODY_25", params, schedule=[prec] * len(params)) as b:
        assert b.precision_schedule() == [prec] * len(params)
        log_b, out_b = forward(b, x)
    assert log_a == log_b
    assert not any("xhi" in k for _, k in log_b)
    assert np.abs(out_a).max() > 0
    np.testing.assert_array_equal(out_a.view(np.uint32), out_b.view(np.uint32))


# ---- 3: nothing survives re-planning -----------------------------------------------------------

@pytest.mark.parametrize("prec", [FP16, SPLIT], ids=["to_fp16", "to_split"])
def test_3_no_stale_state_after_replanning(ctx, body, prec):
    graph, params = body
    x = image(92, (2, 3, 64, 96))
    with scheduled(ctx, "builtin:BODY_25", params, precision=prec) as fresh:
        log_f, out_f = forward(fresh, x)
    with scheduled(ctx, "builtin:BODY_25", params, SCHEDULES["alternating"]) as net:
        _, mixed = forward(net, x)
        assert not np.array_equal(mixed, out_f)
        net.set_precision_schedule([prec] * len(params))
        log, out = forward(net, x)
    assert log == log_f
    np.testing.assert_array_equal(out.view(np.uint32), out_f.view(np.uint32))


# ---- 4: hi-only kernels against the three-product kernels over a zero twin -----------------------

def variant_schedules():
    """{name: ({conv: SPLIT}, conv3w8x instantiations that must run)} on variants_graph: every conv
    named is split, the others fp16."""
    return {
        "first_fp16": (dict.fromkeys(["c2", "c3", "c4", "c5", "c6", "c6b", "c6d", "c6c", "c7"], SPLIT),
                       ("conv3w8x_kernel<128,1,",)),
        # c3 / c5 read the fp16 c2 / c4, c6b the fp16 c6; the split head pair reads the fp16 c6d
        # (conv_head_kernel has no hi-only instantiation: a zero twin)
        "odd": (dict.fromkeys(["c3", "c5", "c6b", "c6c", "c7"], SPLIT),
                ("conv3w8x_kernel<96,1,", "conv3w8x_kernel<128,2,")),
        # c6 reads a concat of two fp16 members, c6d the fp16 c6b
        "even": (dict.fromkeys(["c2", "c4", "c6", "c6d"], SPLIT),
                 ("conv3w8x_kernel<128,1,", "conv3w8x_kernel<128,4,")),
    }


@pytest.mark.parametrize("name", ["first_fp16", "odd", "even"])
def test_4_conv3w8_hi_only(ctx, record_property, name):
    sched, must_run = variant_schedules()[name]
    L = variants_graph()
    graph = prototxt.parse(prototxt.emit(L))
    params = random_params(graph, 87)
    x = image(88, (2, 3, 256, 386))
    with scheduled(ctx, L, params, sched) as net:
        log, out = forward(net, x)
        for prefix in must_run:
            assert any(k.startswith(prefix) and hi_only(k) for _, k in log), (prefix, log)
        blobs = all_blobs(net, graph, (1, 1))
        if name == "first_fp16":   # (the last frame: the references of the 512-channel layers
            # at this size take seconds per frame)
            rows = check_schedule(net, graph, params, x, [1], named(net), log=log)
            print_rows(rows, "4: 2x256x386 first conv fp16")
            record_property("max_frac_of_bound", round(max(r.frac for r in rows), 4))
    with dev_switches(SPLIT_XHI=0), scheduled(ctx, L, params, sched) as net:
        log0, out0 = forward(net, x)
        assert not any("xhi" in k for _, k in log0), log0
        assert [layer for layer, _ in log0] == [layer for layer, _ in log]
        blobs0 = all_blobs(net, graph, (1, 1))
    assert np.abs(out).max() > 0
    assert_equal_values(dict(blobs, net_output=out), dict(blobs0, net_output=out0))


def test_4_conv3_hi_only(ctx, body):
    """The same A/B on conv3_kernel's hi-only instantiations (3x3 tiles of 64, 96 and 128 outputs and
    the 1x1 tiles), BODY_25 alternating by conv index at 2 x 64 x 96."""
    graph, params = body
    x = image(92, (2, 3, 64, 96))
    with scheduled(ctx, "builtin:BODY_25", params, SCHEDULES["alternating"]) as net:
        log, out = forward(net, x)
        xhi = {k for _, k in log if hi_only(k)}
        assert any(k.startswith("conv3_kernel<") and ",3,8,split,xhi>" in k for k in xhi), xhi
        assert any(k.startswith("conv3_kernel<") and ",1,8,split,xhi>" in k for k in xhi) or \
            any(k.startswith("conv3_kernel<") and ",1,16,split,xhi>" in k for k in xhi), xhi
        blobs = all_blobs(net, graph)
    with dev_switches(SPLIT_XHI=0), scheduled(ctx, "builtin:BODY_25", params, SCHEDULES["alternating"]) as net:
        log0, out0 = forward(net, x)
        assert not any("xhi" in k for _, k in log0), log0
        blobs0 = all_blobs(net, graph)
    assert_equal_values(dict(blobs, net_output=out), dict(blobs0, net_output=out0))


# ---- 5: pools ------------------------------------------------------------------------------------

@pytest.mark.parametrize("split_conv", ["c2", "c3"])
def test_5_pools_follow_their_input(ctx, record_property, split_conv):
    L = front_graph()
    graph = prototxt.parse(prototxt.emit(L))
    params = random_params(graph, 81)
    x = image(82, (4, 3, 184, 328))
    got = {}
    for fuse in (1, 0):
        with dev_switches(CONV1_FUSED=0, POOL_FUSE=fuse), scheduled(ctx, L, params, {split_conv: SPLIT}) as net:
            log, out = forward(net, x)
            layers = [layer for layer, _ in log]
            assert ("c2+pool" in layers) == bool(fuse) and ("pool" in layers) == (not fuse), log
            pool_k = [k for layer, k in log if layer == "pool"]
            if not fuse:   # the stand-alone pool follows its input: split iff c2 is
                assert pool_k == ["maxpool2_split_kernel" if split_conv == "c2" else "maxpool2_kernel"], pool_k
            k = conv_instantiations(log, ["c2", "c3"])
            assert k["c2"][0].startswith("conv3w8_kernel<64,1,%d," % fuse), k
            assert k["c2"][0].endswith(",split>") == (split_conv == "c2"), k   # (a zero twin: no 64-output hi-only tile)
            assert hi_only(k["c3"][0]) == (split_conv == "c3"), k
            rows = check_schedule(net, graph, params, x, [0, 3], named(net), log=log)
            print_rows(rows, "5: 4x184x328 %s split POOL_FUSE=%d" % (split_conv, fuse))
            hi, lo, has_lo = net.blob_planes("pool1")
            assert has_lo == (split_conv == "c2")
            assert (np.abs(lo).max() > 0) == (split_conv == "c2")
            got[fuse] = dict(pool1_hi=hi, pool1_lo=lo, net_output=out)
    for name in got[1]:
        np.testing.assert_array_equal(got[1][name].view(np.uint32), got[0][name].view(np.uint32), err_msg=name)


# ---- 6: small-batch tiles ------------------------------------------------------------------------

def test_6_small_batch_bit_identical(ctx, body):
    graph, params = body
    x = image(92, (1, 3, 64, 96))
    outs = {}
    for small in (False, True):
        with scheduled(ctx, "builtin:BODY_25", params, SCHEDULES["alternating"], small=small) as net:
            log, outs[small] = forward(net, x)
            ks = [k for _, k in log]
            assert any(k.startswith("conv3s_kernel<") for k in ks) == small, ks
            if small:
                assert any(k.startswith("conv3s_kernel<") and hi_only(k) for k in ks), ks
                assert any(k.startswith("conv3s_kernel<") and k.endswith(",split>") for k in ks), ks
    assert np.abs(outs[True]).max() > 0
    np.testing.assert_array_equal(outs[True].view(np.uint32), outs[False].view(np.uint32))
