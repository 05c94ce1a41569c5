"""CPU: the per-layer precision schedule's ABI and planner (opk_net_set_precision_schedule,
opk_net_conv_precision, opk_net_conv_kernels) on a host-only context, BODY_25 on a 256-CU chip.

conv_kernels gives the launch-log name of every launch up to the template arguments the planner
fixes: the whole instantiation for conv3_kernel / conv3s_kernel (split: "...,split>", a split conv
over a source without a lo twin: "...,split,xhi>"), "conv3w8_kernel<BN,NB,POOL" for the persistent
8-wave kernel in either precision and "conv3w8x_kernel<BN,NB" for its hi-only variant.
"""
import ctypes

import pytest

from openpose_amd import _lib
from openpose_amd.api import (PRECISION_FP16, PRECISION_SPLIT, Context, Net, OpkError, dev_switches)

CUS = 256
OPK_ERR_ARG = 1
BENCH = (130, 368, 656)
ONE = (1, 368, 656)


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


def kernels(net, shape):
    return [net.conv_kernels(i, *shape, CUS) for i in range(len(net.convs()))]


def trunk(c):
    return not c["name"].startswith("Mconv")


def hi_only(names):
    return any(k.endswith(",split,xhi>") or k.startswith("conv3w8x_kernel<") for k in names)


@pytest.mark.parametrize("shape,small", [(BENCH, False), (ONE, True)], ids=["130x368x656", "1x368x656-small"])
@pytest.mark.parametrize("prec", [PRECISION_FP16, PRECISION_SPLIT], ids=["fp16", "split"])
def test_uniform_schedule_plans_as_set_precision(host, shape, small, prec):
    a, b = Net(host, "builtin:BODY_25"), Net(host, "builtin:BODY_25")
    try:
        for n in (a, b):
            n.set_small_batch(small)
        a.set_precision(prec)
        # (from the other uniform schedule, so that every conv changes)
        b.set_precision_schedule([1 - prec] * len(b.convs()))
        b.set_precision_schedule([prec] * len(b.convs()))
        assert b.precision_schedule() == [prec] * len(b.convs()) == a.precision_schedule()
        ka, kb = kernels(a, shape), kernels(b, shape)
        assert ka == kb
        assert not any(hi_only(k) for k in kb)
        if small:
            assert any(k and k[0].startswith("conv3s_kernel<") for k in kb)
    finally:
        a.close()
        b.close()


def test_fp16_trunk_split_stages(host, net):
    convs = net.convs()
    ref = Net(host, "builtin:BODY_25")
    try:
        fp16 = kernels(ref, BENCH)
    finally:
        ref.close()
    net.set_precision_schedule(lambda c: PRECISION_FP16 if trunk(c) else PRECISION_SPLIT)
    got = kernels(net, BENCH)
    assert got[0] == ["conv1_fused_kernel"] and got[1] == []
    for i, c in enumerate(convs):
        if trunk(c):
            assert got[i] == fp16[i], c["name"]
    # the whole input of stage 0's first conv is conv4_4_CPM, trunk output; every later stage
    # reads a concat with a split member, every other conv a split blob
    first = {"Mconv1_stage0_L2_0"}
    assert [c["cin"] for c in convs if c["name"] in first] == [128]
    for i, c in enumerate(convs):
        if trunk(c):
            continue
        assert net.precision_schedule()[i] == PRECISION_SPLIT
        assert hi_only(got[i]) == (c["name"] in first), (c["name"], got[i])
        for k in got[i]:
            if k.startswith(("conv3_kernel<", "conv3s_kernel<")):
                assert ",split" in k, (c["name"], k)
            else:   # the persistent kernel (the prefix carries no precision) or a fused head pair
                assert k.startswith(("conv3w8_kernel<", "conv3w8x_kernel<")) or k == "conv_head_kernel", k
    # at the bench batch the hi-only convs run the persistent kernel's variant; one frame in
    # small-batch mode takes the generic kernel's
    assert all(got[i] and got[i][0].startswith("conv3w8x_kernel<") for i, c in enumerate(convs)
               if c["name"] in first)
    net.set_small_batch(True)
    one = kernels(net, ONE)
    for i, c in enumerate(convs):
        if not trunk(c):
            assert hi_only(one[i]) == (c["name"] in first), (c["name"], one[i])
        if c["name"] in first:
            assert one[i][0].startswith(("conv3s_kernel<", "conv3_kernel<")) and one[i][0].endswith(",split,xhi>")
    # SPLIT_XHI=0: the three-product kernels everywhere
    with dev_switches(SPLIT_XHI=0):
        assert not any(hi_only(k) for k in kernels(net, ONE) + kernels(net, BENCH))


def test_head_pairs(net):
    convs = net.convs()
    names = [c["name"] for c in convs]
    m6 = [i for i, n in enumerate(names) if n.startswith("Mconv6_")]
    assert m6 and all(names[i + 1].startswith("Mconv7_") for i in m6)
    sched = [PRECISION_FP16] * len(convs)
    mixed, split_pair = m6[0], m6[1]
    sched[mixed] = PRECISION_SPLIT                      # Mconv6 split, Mconv7 fp16
    sched[split_pair] = sched[split_pair + 1] = PRECISION_SPLIT
    net.set_precision_schedule(sched)
    for shape in (BENCH, ONE):
        got = kernels(net, shape)
        # a mixed pair: two launches, each of its own precision (the 1x1 Mconv6 over an fp16
        # source is hi-only)
        assert len(got[mixed]) >= 1 and all(k.startswith("conv3_kernel<") and k.endswith(",split,xhi>")
                                            for k in got[mixed]), got[mixed]
        assert len(got[mixed + 1]) >= 1 and all(k.startswith("conv3_kernel<") and "split" not in k
                                                for k in got[mixed + 1]), got[mixed + 1]
        # equal precisions: the fused kernel on the pair's first conv
        assert got[split_pair] == ["conv_head_kernel"] and got[split_pair + 1] == []
        for i in m6[2:]:
            assert got[i] == ["conv_head_kernel"] and got[i + 1] == []
    sched[mixed], sched[mixed + 1] = PRECISION_FP16, PRECISION_SPLIT   # the other way round
    net.set_precision_schedule(sched)
    got = kernels(net, ONE)
    assert all("split" not in k for k in got[mixed]) and got[mixed]
    assert all(k.endswith(",split,xhi>") for k in got[mixed + 1]) and got[mixed + 1]


def test_refusals_leave_the_schedule(net):
    L = _lib.load()
    n = len(net.convs())
    sched = [i % 2 for i in range(n)]
    net.set_precision_schedule(sched)
    assert net.precision_schedule() == sched
    with pytest.raises(OpkError):
        net.set_precision_schedule(sched[:-1])
    assert net.precision_schedule() == sched
    bad = [PRECISION_SPLIT] * n
    bad[17] = 2
    with pytest.raises(OpkError) as e:
        net.set_precision_schedule(bad)
    assert "17" in str(e.value), str(e.value)
    assert net.precision_schedule() == sched
    arr = (ctypes.c_int * n)(*bad)
    assert L.opk_net_set_precision_schedule(net.h, arr, n) == OPK_ERR_ARG
    assert b"index 17" in L.opk_last_error()
    assert L.opk_net_set_precision_schedule(net.h, arr, n + 1) == OPK_ERR_ARG
    assert L.opk_net_set_precision_schedule(None, arr, n) == OPK_ERR_ARG
    assert L.opk_net_set_precision_schedule(net.h, None, n) == OPK_ERR_ARG
    assert net.precision_schedule() == sched
    assert L.opk_net_conv_precision(None, 0) == -1
    assert L.opk_net_conv_precision(net.h, -1) == -1 and L.opk_net_conv_precision(net.h, n) == -1
    # set_precision keeps its refusals
    with pytest.raises(OpkError):
        net.set_precision(2)
    assert net.precision_schedule() == sched


def test_set_precision_restores_uniform(host, net):
    n = len(net.convs())
    fresh = kernels(net, BENCH)
    net.set_precision_schedule([i % 2 for i in range(n)])
    assert kernels(net, BENCH) != fresh
    net.set_precision(PRECISION_FP16)
    assert net.precision_schedule() == [PRECISION_FP16] * n
    assert kernels(net, BENCH) == fresh
    net.set_precision_schedule([i % 2 for i in range(n)])
    net.set_precision(PRECISION_SPLIT)
    assert net.precision_schedule() == [PRECISION_SPLIT] * n
    ref = Net(host, "builtin:BODY_25")
    try:
        ref.set_precision(PRECISION_SPLIT)
        assert kernels(net, BENCH) == kernels(ref, BENCH)
    finally:
        ref.close()


def test_dict_and_callable_forms(net):
    convs = net.convs()
    want = [PRECISION_FP16 if trunk(c) else PRECISION_SPLIT for c in convs]
    net.set_precision_schedule(want)
    listed = kernels(net, ONE)
    net.set_precision(PRECISION_FP16)
    net.set_precision_schedule(lambda c: PRECISION_FP16 if trunk(c) else PRECISION_SPLIT)
    assert net.precision_schedule() == want and kernels(net, ONE) == listed
    net.set_precision(PRECISION_FP16)
    net.set_precision_schedule({c["name"]: PRECISION_SPLIT for c in convs if not trunk(c)})
    assert net.precision_schedule() == want and kernels(net, ONE) == listed
    # convs a dict does not name keep their value
    net.set_precision_schedule({"conv1_1": PRECISION_SPLIT})
    assert net.precision_schedule() == [PRECISION_SPLIT] + want[1:]
    with pytest.raises(OpkError):
        net.set_precision_schedule({"no_such_conv": PRECISION_SPLIT})
    # the callable sees the conv's index too
    net.set_precision_schedule(lambda c: c["index"] % 2)
    assert net.precision_schedule() == [i % 2 for i in range(len(convs))]
