"""CPU: the small-batch net mode on the 7x7 CPM nets (face, hand, COCO_18, MPI) -- the planner
(conv_plan.cpp) through Net.conv_plan / Net.conv_kernels on a host-only context, 256 CUs.

These nets carry a 3-pixel zero border (their 7x7 stage layers pad 3).  One 368 x 368 crop gives the
25 7x7 layers of a face / hand net ceil(46 * 52 / 256) = 10 workgroups of conv3_kernel<256,..,7>
each, one 368 x 656 COCO frame ceil(46 * 88 / 256) = 16.  With the mode on they take conv3s_kernel's
7x7 tiles (64 x 32 under a 384-row halo, 128 x 64 under 448 rows), and the under-filled 3x3 layers
the 3x3 tiles at border 3.  `workgroups` is the planner's fill measure: tiles of the
n x h x (w + 2 border) GEMM positions times n-blocks.
"""
import pytest

from openpose_amd.api import PRECISION_SPLIT, Context, Net

CUS = 256
CAP = 4        # conv.h kConv3sMaxPerCu: no small tiles beyond this many workgroups per CU
BORDER = 3
ONE = [("builtin:FACE", (1, 368, 368), 10), ("builtin:HAND", (1, 368, 368), 10),
       ("builtin:COCO_18", (1, 368, 656), 16)]
FULL = [("builtin:FACE", (32, 368, 368)), ("builtin:HAND", (32, 368, 368)),
        ("builtin:COCO_18", (64, 368, 656))]


def ceil_div(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def host():
    c = Context.host_only()
    yield c
    c.close()


def plans(net, shape):
    return [dict(c, **net.conv_plan(i, *shape, CUS)) for i, c in enumerate(net.convs())]


def both(host, model, shape, split=False):
    """(mode-off plans, mode-on plans, mode-on kernels) of every conv."""
    net = Net(host, model)
    try:
        if split:
            net.set_precision(PRECISION_SPLIT)
        off = plans(net, shape)
        net.set_small_batch(True)
        on = plans(net, shape)
        kernels = [net.conv_kernels(i, *shape, CUS) for i in range(len(on))]
    finally:
        net.close()
    return off, on, kernels


def stage_tiles(shape, bm, bn, cout):
    """The fill measure of a conv at the 1/8 level (where every 7x7 layer of these nets runs)."""
    n, h, w = shape
    return ceil_div(n * (h // 8) * (w // 8 + 2 * BORDER), bm) * ceil_div(cout, bn)


@pytest.mark.parametrize("model,shape,wg7", ONE, ids=[m.split(":")[1] for m, _, _ in ONE])
def test_mode_off_pins_todays_plan(host, model, shape, wg7):
    off, _, _ = both(host, model, shape)
    assert not any(c["small"] for c in off)
    k7 = [c for c in off if c["kernel_size"] == 7]
    assert len(k7) == (50 if "COCO" in model else 25)
    for c in k7:
        assert (c["bm"], c["workgroups"]) == (256, wg7), c
        assert c["workgroups"] == stage_tiles(shape, 256, c["bn"], c["num_output"]), c


@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
@pytest.mark.parametrize("model,shape,wg7", ONE, ids=[m.split(":")[1] for m, _, _ in ONE])
def test_mode_on_one_crop(host, model, shape, wg7, split):
    off, on, kernels = both(host, model, shape, split)
    n7 = 0
    for a, b, ks in zip(off, on, kernels):
        image = b["name"] == "conv1_1"
        k = b["kernel_size"]
        if k == 7 or (k == 3 and not image and a["workgroups"] < CUS):
            assert b["small"] == 1, (a, b)
            assert a["workgroups"] < b["workgroups"] <= CAP * CUS, (a, b)
            assert len(ks) == 1 and ks[0].startswith("conv3s_kernel<%d,%d," % (b["bm"], b["bn"])), (b, ks)
            assert ks[0].endswith(",split>") == split, ks
            # the instantiation carries the kernel size of a 7x7 conv
            assert (",7,7" in ks[0]) == (k == 7), ks
        else:   # every 1x1 conv, the image conv and the 3x3 convs that fill the chip: as without the mode
            assert b == a, (a, b)
            assert not any(x.startswith("conv3s_kernel") for x in ks), (b, ks)
        if k == 1 or image:
            assert b["small"] == 0, b
        if k == 7:
            n7 += 1
            assert b["num_output"] == 128, b
            # one crop: 38 m-tiles of 64 positions by 4 n-blocks of 32 outputs; one COCO frame: the
            # 128 x 64 tile gives a workgroup per four CUs (32 m-tiles by 2 n-blocks)
            tile = (128, 64) if "COCO" in model else (64, 32)
            assert (b["bm"], b["bn"]) == tile, b
            assert b["workgroups"] == stage_tiles(shape, *tile, 128) == (64 if "COCO" in model else 152), b
            if "COCO" not in model:
                assert b["workgroups"] >= CUS // 2, b
            assert ks[0].startswith("conv3s_kernel<%d,%d,%d,7,7" % (tile + (448 if tile[0] == 128 else 384, ))), ks
    assert n7 == (50 if "COCO" in model else 25)
    # the VGG / CPM 3x3 front at the 1/8 level runs small at border 3
    by = {c["name"]: c for c in on}
    assert by["conv4_2"]["small"] == 1 and by["conv4_2"]["kernel_size"] == 3


def test_mode_on_larger_tile_from_two_crops(host):
    """The 128 x 64 7x7 tile from a workgroup per four CUs (conv.h kConv7sBigPerCus, measured): two
    crops give 38 x 2 = 76, one crop 19 x 2 = 38 (the 64 x 32 tile, above)."""
    for n, wg in ((2, 76), (4, 150), (8, 300)):
        shape = (n, 368, 368)
        _, on, kernels = both(host, "builtin:FACE", shape)
        for b, ks in zip(on, kernels):
            if b["kernel_size"] == 7:
                assert (b["small"], b["bm"], b["bn"]) == (1, 128, 64), b
                assert b["workgroups"] == stage_tiles(shape, 128, 64, 128) == wg >= CUS // 4, b
                assert ks == ["conv3s_kernel<128,64,448,7,7>"], ks


@pytest.mark.parametrize("model,shape", FULL, ids=[m.split(":")[1] for m, _ in FULL])
def test_full_batches_unchanged(host, model, shape):
    off, on, kernels = both(host, model, shape)
    filled = 0
    for a, b, ks in zip(off, on, kernels):
        if a["workgroups"] >= CUS or b["kernel_size"] == 1 or b["name"] == "conv1_1":
            assert b == a, (a, b)
            assert not any(x.startswith("conv3s_kernel") for x in ks), (b, ks)
            filled += a["kernel_size"] == 7
    assert filled >= 1   # (the 7x7 layers themselves fill the chip at these batches)


def test_mpi_nets_take_the_mode(host):
    for model in ("builtin:MPI_15", "builtin:MPI_15_4"):
        off, on, _ = both(host, model, (1, 368, 656))
        k7 = [(a, b) for a, b in zip(off, on) if b["kernel_size"] == 7]
        assert k7 and all(a["small"] == 0 and b["small"] == 1 for a, b in k7), model


@pytest.mark.parametrize("shape", [(1, 368, 656), (2, 64, 96)], ids=["1x368x656", "2x64x96"])
def test_body25_names_unchanged(host, shape):
    """BODY_25 (border 1, no 7x7): the small tiles and their names as before."""
    _, on, kernels = both(host, "builtin:BODY_25", shape)
    names = {ks[0] for b, ks in zip(on, kernels) if b["small"]}
    assert names and names <= {"conv3s_kernel<64,32,256,9>", "conv3s_kernel<128,64,320,3>"}, names
    assert "conv3s_kernel<64,32,256,9>" in names
