"""CPU: the small-batch net mode's ABI and planner (opk_net_set_small_batch, opk_net_conv_plan) on
a host-only context.

BODY_25 at one 368 x 656 frame on a 256-CU chip: conv3_shape's 256 / 512-position tiles give the
90 stage 3x3 layers (46 x 82, 96 or 128 outputs) 16 workgroups each; with the mode on they take
conv3s tiles and at least a workgroup per two CUs.  The bench batch (130 frames) plans the same
either way.  `workgroups` is the planner's fill measure: tiles of the n x h x (w + 2) GEMM positions
times n-blocks.
"""
import ctypes

import pytest

from openpose_amd import _lib
from openpose_amd.api import Context, Net

CUS = 256
OPK_ERR_ARG = 1


@pytest.fixture(scope="module")
def host():
    c = Context.host_only()
    yield c
    c.close()


@pytest.fixture()
def net(host):
    n = Net(host, "builtin:BODY_25")
    yield n
    n.close()


def plans(net, n, h, w):
    return [dict(c, **net.conv_plan(i, n, h, w, CUS)) for i, c in enumerate(net.convs())]


def stage_3x3(c):
    return c["name"].startswith("Mconv") and c["kernel_size"] == 3


def level3_3x3(c):
    """3x3 convs at the 46 x 82 level: everything after pool3."""
    return c["kernel_size"] == 3 and (c["name"].startswith(("Mconv", "conv4_")))


def test_abi_setter_getter(net):
    L = _lib.load()
    assert L.opk_net_small_batch(net.h) == 0          # off by default
    assert L.opk_net_small_batch(None) == -1
    assert L.opk_net_set_small_batch(net.h, 1) == 0
    assert L.opk_net_small_batch(net.h) == 1
    for bad in (2, -1):
        assert L.opk_net_set_small_batch(net.h, bad) == OPK_ERR_ARG
        assert b"small batch" in L.opk_last_error()
        assert L.opk_net_small_batch(net.h) == 1      # unchanged by a refused value
    assert L.opk_net_set_small_batch(net.h, 0) == 0
    assert L.opk_net_small_batch(net.h) == 0
    assert L.opk_net_set_small_batch(None, 1) == OPK_ERR_ARG


def test_python_round_trip(net):
    assert net.small_batch is False
    net.set_small_batch(True)
    assert net.small_batch is True
    net.set_small_batch(False)
    assert net.small_batch is False


def test_conv_plan_arguments(net):
    L = _lib.load()
    v = ctypes.c_int()
    n = len(net.convs())
    for args in ((-1, 1, 368, 656, CUS), (n, 1, 368, 656, CUS), (0, 0, 368, 656, CUS), (0, 1, 368, 656, 0)):
        assert L.opk_net_conv_plan(net.h, *args, ctypes.byref(v), None, None, None) == OPK_ERR_ARG
    assert L.opk_net_conv_plan(net.h, 1, 1, 368, 656, CUS, None, None, None, None) == 0   # NULL outputs


def test_flag_off_pins_todays_planner(net):
    p = plans(net, 1, 368, 656)
    stage = [c for c in p if stage_3x3(c)]
    assert len(stage) == 90
    for c in stage:
        assert (c["small"], c["bm"], c["workgroups"]) == (0, 256, 16), c
        assert c["bn"] == (96 if c["num_output"] == 96 else 128), c
    by = {c["name"]: c for c in p}
    for name in ("conv4_1", "conv4_2"):
        assert (by[name]["small"], by[name]["workgroups"]) == (0, 64), by[name]
    for name in ("conv3_1", "conv3_2", "conv3_3", "conv3_4"):
        assert (by[name]["small"], by[name]["workgroups"]) == (0, 120), by[name]
    assert not any(c["small"] for c in p)


def test_flag_on_one_frame(net):
    off = plans(net, 1, 368, 656)
    net.set_small_batch(True)
    on = plans(net, 1, 368, 656)
    assert sum(stage_3x3(c) for c in on) == 90
    nsmall = 0
    for a, b in zip(off, on):
        image = b["name"] == "conv1_1"
        if b["kernel_size"] == 3 and not image and a["workgroups"] < CUS:
            assert b["small"] == 1 and b["workgroups"] > a["workgroups"], (a, b)
            nsmall += 1
        else:   # everything else as without the mode
            assert b == a, (a, b)
        if b["kernel_size"] == 1 or image:
            assert b["small"] == 0, b
        if level3_3x3(b) and b["num_output"] in (96, 128):
            assert b["small"] == 1 and b["workgroups"] >= CUS // 2, b
    assert nsmall >= 90 + 4 + 4   # the stages, conv4_*, conv3_*
    # the example geometry: 61 m-tiles of 64 positions x 3 or 4 n-blocks of 32 outputs
    by = {c["name"]: c for c in on}
    assert (by["Mconv1_stage0_L2_0"]["bm"], by["Mconv1_stage0_L2_0"]["bn"]) == (64, 32)
    assert {c["workgroups"] for c in on if stage_3x3(c)} == {183, 244}


def test_flag_on_bench_batch_unchanged(net):
    off = plans(net, 130, 368, 656)
    net.set_small_batch(True)
    assert plans(net, 130, 368, 656) == off
    assert not any(c["small"] for c in off)


def test_fused_first_layers_keep_their_plan(net):
    """conv1_2 runs inside conv1_fused_kernel in fp16 (even sizes): never a conv3s launch, however
    few tiles its own geometry would give."""
    net.set_small_batch(True)
    by = {c["name"]: c for c in plans(net, 1, 64, 96)}
    assert by["conv1_2"]["small"] == 0 and by["conv1_1"]["small"] == 0
    assert by["conv2_1"]["small"] == 1
