"""GPU: the host-side query and the launchers agree -- the launch log of one real forward, per
conv, equals Net.conv_kernels entry by entry (the launchers log names built from the plan's
prefix).  Small shapes only; which kernels the shapes that matter take is
tests/test_conv_dispatch.py's (CPU) business.
"""
import numpy as np
import pytest
import torch

from openpose_amd.api import PRECISION_SPLIT, Net, dev_switches
from tests.conv_dispatch_cases import FLIPS, case, graph_of, model_path
from tests.launch_check import random_params
from tests.test_conv_dispatch import RECORDED, expected, matches

pytestmark = pytest.mark.gpu


def run(ctx, model, shape, split=False, small=False, **switches):
    n, h, w = shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    with model_path(model) as path, dev_switches(LAUNCH_LOG=1, **switches):
        net = Net(ctx, path)
        try:
            net.set_params(random_params(graph_of(model), 71))
            if split:
                net.set_precision(PRECISION_SPLIT)
            if small:
                net.set_small_batch(True)
            net.forward(torch.zeros((n, 3, h, w), device="cuda"))
            ctx.sync()
            names = [c["name"] for c in net.convs()]
            want = expected(net.launch_log(), names)
            got = {name: net.conv_kernels(i, n, h, w, cus) for i, name in enumerate(names)}
        finally:
            net.close()
    for name in names:
        assert len(got[name]) == len(want[name]) and all(map(matches, got[name], want[name])), \
            (name, got[name], want[name])
    return got


@pytest.mark.parametrize("small", [False, True], ids=["plain", "small"])
@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
def test_body25_log_equals_query(ctx, split, small):
    got = run(ctx, "builtin:BODY_25", (2, 64, 96), split, small)
    assert any(k.startswith("conv3s_kernel<") for ks in got.values() for k in ks) == small


def test_front_graph_unfused_log_equals_query(ctx):
    got = run(ctx, "front", (1, 16, 36), CONV1_FUSED=0)
    assert got["c1"] == ["conv_image_kernel"] and len(got["c2"]) == 1


@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
def test_a_planned_shape_keeps_its_launches_when_a_switch_flips(ctx, split):
    """A decision switch is read when a shape is planned and holds for that plan: a net that has
    forwarded a shape launches the same kernels, to the same bits, while CONV3W8_64,
    CONV3_PERSIST, CONV3_W16, CONV3_SMALL (and, in split precision, SPLIT_XHI) are flipped; a net
    built inside the flip takes the flipped decision -- the launch log recorded for that switch
    set -- and computes the same bits (the tile variants are bit-identical).  The front graph at
    4 x 184 x 328 without the conv1 fusion: the shape of the recorded flip cases, at which
    CONV3W8_64, CONV3_PERSIST and CONV3_W16 each change what a fresh net launches (CONV3_SMALL does
    not at this size, nor SPLIT_XHI under a uniform schedule, which has no hi-only conv)."""
    shape, fixed = (4, 184, 328), dict(CONV1_FUSED=0)
    params = random_params(graph_of("front"), 7)   # (the recorded logs' parameters)
    x = torch.from_numpy(np.random.default_rng(5).uniform(-0.5, 0.5, (shape[0], 3) + shape[1:])
                         .astype(np.float32)).cuda()

    def forwarded(path):
        net = Net(ctx, path)
        try:
            net.set_params(params)
            if split:
                net.set_precision(PRECISION_SPLIT)
            return net, again(net)
        except Exception:
            net.close()
            raise

    def again(net):
        net.forward(x)
        ctx.sync()
        return [list(e) for e in net.launch_log()], net.output_numpy()

    with model_path("front") as path, dev_switches(LAUNCH_LOG=1, **fixed):
        net, (log, out) = forwarded(path)
        changed = []
        try:
            assert log == RECORDED[case("front", shape, split, **fixed)["name"]]["log"]
            for flip in FLIPS + ([dict(SPLIT_XHI=0)] if split else []):
                with dev_switches(**flip):
                    log1, out1 = again(net)
                    assert log1 == log, (flip, log1, log)
                    assert np.array_equal(out1, out), flip
                    fresh, (log2, out2) = forwarded(path)
                    fresh.close()
                    if "SPLIT_XHI" in flip:   # (a uniform schedule has no hi-only conv: nothing to change)
                        assert log2 == log
                    else:
                        assert log2 == RECORDED[case("front", shape, split, **fixed, **flip)["name"]]["log"], flip
                    changed += [k for k in flip if log2 != log]
                    assert np.array_equal(out2, out), flip
                assert again(net)[0] == log
            # the flips that do change what a fresh net launches at this shape
            assert changed == ["CONV3W8_64", "CONV3_PERSIST", "CONV3_W16"]
        finally:
            net.close()
