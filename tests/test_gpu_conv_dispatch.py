"""GPU: the host-side query and the launchers agree -- the launch log of one real forward, per
conv, equals Net.conv_kernels entry by entry (the launchers log names built from the plan's
prefix).  Small shapes only; which kernels the shapes that matter take is
tests/test_conv_dispatch.py's (CPU) business.
"""
import pytest
import torch

from openpose_amd.api import PRECISION_SPLIT, Net, dev_switches
from tests.conv_dispatch_cases import graph_of, model_path
from tests.launch_check import random_params
from tests.test_conv_dispatch import expected, matches

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
