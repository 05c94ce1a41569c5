"""CPU: the channel matrix (tests/channel_matrix_cases.py) against the host-side planner
(Net.conv_kernels on a host-only context, 256 CUs): every case of tests/test_gpu_channel_matrix.py
is planned onto the kernel instantiation it exists for, so a planner change cannot silently empty
a case; and the graphs the library cannot run are refused when the net is built, with a message
that names the layer.
"""
import pytest

from openpose_amd.api import PRECISION_SPLIT, Context, Net
from tests import prototxt
from tests.channel_matrix_cases import (CUS, FIRST_REFUSED, FUSED_HEADS, OFFGRID_SMALL_MODE, UNFUSED_HEADS,
                                        all_cases, first_graph, instantiation, offgrid_graph, pool_graph)


@pytest.fixture(scope="module")
def host():
    c = Context.host_only()
    yield c
    c.close()


def build(host, layers, tmp_path, split=False, small=False):
    path = tmp_path / "net.prototxt"
    path.write_text(prototxt.emit(layers))
    net = Net(host, str(path))
    if split:
        net.set_precision(PRECISION_SPLIT)
    net.set_small_batch(small)
    return net


def kernels(net, shape):
    return {c["name"]: net.conv_kernels(i, *shape, CUS) for i, c in enumerate(net.convs())}


@pytest.mark.parametrize("case", all_cases(), ids=lambda c: c["name"])
def test_planned_onto_the_instantiation(host, tmp_path, case):
    net = build(host, case["graph"](*case["args"]), tmp_path, case["split"], case["small"])
    try:
        got = kernels(net, case["shape"])
        assert case["must_run"], case["name"]
        for name, prefix in case["must_run"].items():
            if prefix is None:   # inside the kernel of the conv before it
                assert got[name] == [], (name, got)
                continue
            assert len(got[name]) == 1 and instantiation(got[name][0], prefix, case["split"]), \
                (name, got[name], prefix)
    finally:
        net.close()


def test_matrix_covers_what_it_must():
    cases = all_cases()
    wanted = [p for c in cases for p in c["must_run"].values() if p]
    for prefix in ("conv3_kernel<256,96,512,3,1,3", "conv3_kernel<256,128,512,3,1,3",
                   "conv3_kernel<512,128,704,3,1,3,16", "conv3_kernel<256,256,256,1,1,1,16",
                   "conv3_kernel<512,64,768,3,1,3", "conv3_kernel<256,96,256,1,2,1",
                   "conv3_kernel<256,128,1024,1,1,7", "conv3_kernel<256,64,1024,1,1,7",
                   "conv3s_kernel<64,32,256,9", "conv3s_kernel<128,64,320,3", "conv3s_kernel<64,32,384,7,7",
                   "conv_head_kernel", "conv_image_kernel"):
        assert prefix in wanted, prefix
    assert {(n1, n2) for n1, n2, _ in FUSED_HEADS} == {(256, 1), (256, 32), (256, 33), (512, 64)}
    assert (256, 33, True) in FUSED_HEADS
    assert set(UNFUSED_HEADS) == {(512, 65), (128, 26), (384, 26)}
    for name in ("offgrid", "odd", "first 4", "first 32", "first 48", "pool 40", "pool 72", "pool 96",
                 "pool 160"):
        for precision in ("fp16", "split"):
            assert any(c["name"].startswith(name + " ") and precision in c["name"] for c in cases), name


def test_small_mode_changes_only_what_it_names(host, tmp_path):
    """The small-batch cases: with the mode off none of the layers runs on conv3s_kernel (the
    bit-identity the GPU test asserts compares two different kernels)."""
    net = build(host, offgrid_graph(), tmp_path)
    try:
        for shape in OFFGRID_SMALL_MODE:
            assert not any(k.startswith("conv3s") for ks in kernels(net, shape).values() for k in ks)
    finally:
        net.close()


@pytest.mark.parametrize("k", FIRST_REFUSED)
def test_first_conv_the_image_kernel_cannot_run_is_refused(host, tmp_path, k):
    """More than 64 outputs, or a count that is no multiple of 4: conv_image_kernel cannot run it
    (launch_conv_image), so the net is refused when it is built -- not at its first forward, after
    conv_kernels has reported conv_image_kernel for it."""
    with pytest.raises(Exception) as e:
        build(host, first_graph(k), tmp_path).close()
    msg = str(e.value)
    assert "c1" in msg and "64" in msg and "multiple of 4" in msg and str(k) in msg, msg


@pytest.mark.parametrize("k", [40, 72])
def test_pool_of_channels_off_the_32_grid_is_planned(host, tmp_path, k):
    """conv -> 2x2 pool -> conv with 40 or 72 pooled channels used to fail with "c3: no readable
    placement of p1": the pool's buffers now have the channel stride the reading conv needs."""
    net = build(host, pool_graph(k), tmp_path)
    try:
        got = kernels(net, (2, 25, 41))
        assert all(len(ks) == 1 for ks in got.values()), got
        by = {c["name"]: c for c in net.convs()}
        assert by["c3"]["num_output"] == 64 and by["c2"]["num_output"] == k
    finally:
        net.close()
