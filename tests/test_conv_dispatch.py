"""CPU: which kernel runs every conv (Net.conv_kernels, the host-side planner conv_plan.cpp) on a
host-only context, against tests/golden/conv_dispatch_parent.json -- the launch logs of real forwards
recorded by tools/record_conv_dispatch.py at the commit before the planner had one home.  The cases
(tests/conv_dispatch_cases.py): BODY_25 at the bench batch, one frame, small, odd and multi-scale
sizes in both precisions and with the small-batch flag; the graphs, shapes and switch sets of
tests/test_gpu_launch_matrix.py's cases a-e and g; a batch whose conv1_2 runs as two frame runs; the
decision switches CONV3W8_64, CONV3_PERSIST, CONV3_W16 and CONV3_SMALL flipped one at a time.
"""
import json
import os
import re

import pytest

from openpose_amd.api import PRECISION_SPLIT, Context, Net, dev_switches
from tests.conv_dispatch_cases import BODY_25, FLIPS, FRAME_RUN_BATCH, case, cases, model_path

with open(os.path.join(os.path.dirname(__file__), "golden", "conv_dispatch_parent.json")) as f:
    TABLE = json.load(f)
CUS = TABLE["cus"]
RECORDED = {c["name"]: c for c in TABLE["cases"]}
PERSISTENT = re.compile(r"conv3w8_kernel<(\d+),\d+,[01]$|conv3w_kernel<(\d+)$|conv3p_kernel<(\d+)$")
TILED = re.compile(r"(conv3s?)_kernel<(\d+),(\d+),.*>$")
BARE = ("conv_image_kernel", "conv1_fused_kernel", "conv_head_kernel")


@pytest.fixture(scope="module")
def host():
    c = Context.host_only()
    yield c
    c.close()


def expected(log, names):
    """{conv: kernels the log shows for it}: those of the entries it leads; none inside another
    conv's fused kernel."""
    out = {}
    for layer, kernel in log:
        members = [m for m in layer.split("+") if m != "pool"]
        if not members:
            continue
        out.setdefault(members[0], []).append(kernel)
        for m in members[1:]:
            out.setdefault(m, [])
    assert sorted(out) == sorted(names), (sorted(out), sorted(names))
    return out


def matches(prefix, logged):
    if TILED.match(prefix):          # the whole instantiation
        return logged == prefix
    if PERSISTENT.match(prefix):     # up to the parameters the plan fixes
        return logged.startswith(prefix + ",")
    return prefix in BARE and (logged == prefix or logged.startswith(prefix + "<"))


def tile_of(prefix):
    """(bm, bn, small) a prefix stands for, None for the kernels without a conv3 plan."""
    m = TILED.match(prefix)
    if m:
        return int(m.group(2)), int(m.group(3)), int(m.group(1) == "conv3s")
    m = PERSISTENT.match(prefix)
    if m:
        return 512, int(next(g for g in m.groups() if g)), 0
    return (0, 0, 0) if prefix == "conv_image_kernel" else None


@pytest.mark.parametrize("case", cases(), ids=lambda c: c["name"])
def test_conv_kernels_match_the_recorded_launch_log(host, case):
    rec = RECORDED[case["name"]]
    assert {k: rec[k] for k in case} == case   # the table was recorded for these cases
    n, h, w = case["shape"]
    with model_path(case["model"]) as path, dev_switches(**case["switches"]):
        net = Net(host, path)
        try:
            if case["split"]:
                net.set_precision(PRECISION_SPLIT)
            if case["small"]:
                net.set_small_batch(True)
            convs = net.convs()
            want = expected(rec["log"], [c["name"] for c in convs])
            for i, c in enumerate(convs):
                got = net.conv_kernels(i, n, h, w, CUS)
                assert len(got) == len(want[c["name"]]), (c["name"], got, want[c["name"]])
                for g, k in zip(got, want[c["name"]]):
                    assert matches(g, k), (c["name"], got, want[c["name"]])
                    tile = tile_of(g)
                    if tile is not None:
                        p = net.conv_plan(i, n, h, w, CUS)
                        assert (p["bm"], p["bn"], p["small"]) == tile, (c["name"], g, p)
        finally:
            net.close()


def test_table_covers_what_it_must():
    names = set(RECORDED)
    assert {c["name"] for c in cases()} <= names
    kernels = {k for c in TABLE["cases"] for _, k in c["log"]}
    for family in ("conv3_kernel<", "conv3p_kernel<", "conv3w_kernel<", "conv3w8_kernel<", "conv3s_kernel<",
                   "conv_image_kernel", "conv1_fused_kernel<", "conv_head_kernel<"):
        assert any(k.startswith(family) for k in kernels) or family == "conv3p_kernel<", family
    # the frame-run case: conv1_2 (with its pool) in two launches
    runs = RECORDED["BODY_25 %dx368x656 split" % FRAME_RUN_BATCH]["log"]
    assert [layer for layer, _ in runs].count("conv1_2+pool") == 2
    for flip in FLIPS:
        (key, value), = flip.items()
        assert sum("%s=%d" % (key, value) in name for name in names) >= 3


def agrees(net, shape, recorded_name):
    names = [c["name"] for c in net.convs()]
    want = expected(RECORDED[recorded_name]["log"], names)
    for i, name in enumerate(names):
        got = net.conv_kernels(i, *shape, CUS)
        assert len(got) == len(want[name]) and all(map(matches, got, want[name])), \
            (recorded_name, name, got, want[name])


@pytest.mark.parametrize("model,shape,split,fixed", [
    ("variants", (2, 256, 386), False, {}),
    ("front", (4, 184, 328), False, dict(CONV1_FUSED=0)),
    ("front", (4, 184, 328), True, dict(CONV1_FUSED=0))], ids=["variants", "front-fp16", "front-split"])
def test_asked_again_after_a_switch_flips(host, model, shape, split, fixed):
    """One net asked again while a decision switch is flipped: the recorded answer of that
    switch set, and the defaults' answer again afterwards.  The switches are read per query (every
    conv_kernels / conv_plan call plans afresh on the host).  A forward is another matter: it
    replays the launches planned when its input shape was first seen, under the switches of that
    moment (tests/test_gpu_conv_dispatch.py)."""
    def name(**switches):
        return case(model, shape, split, **switches)["name"]

    with model_path(model) as path:
        net = Net(host, path)
    try:
        if split:
            net.set_precision(PRECISION_SPLIT)
        with dev_switches(**fixed):
            agrees(net, shape, name(**fixed))
            for flip in FLIPS:
                with dev_switches(**flip):
                    agrees(net, shape, name(**fixed, **flip))
                agrees(net, shape, name(**fixed))
    finally:
        net.close()


@pytest.mark.parametrize("shape,split,small", [((FRAME_RUN_BATCH, 368, 656), True, False),
                                               ((1, 368, 656), False, True)], ids=["frame-runs", "small"])
def test_one_kernel_name_per_frame_run(host, shape, split, small):
    """The run list as data: conv_kernels gives one name per frame run of a conv that launches a
    halo kernel -- k names stand for k even runs of ceil(n / k) frames, the last one the rest --
    each name what a fresh query at that run's frame count gives on its own (name and tile), and
    no smaller number of even runs fits a launch's position range."""
    n, h, w = shape
    net = Net(host, BODY_25)
    try:
        if split:
            net.set_precision(PRECISION_SPLIT)
        if small:
            net.set_small_batch(True)
        several = []
        for i, c in enumerate(net.convs()):
            got = net.conv_kernels(i, n, h, w, CUS)
            if not got or got[0] in BARE:   # inside / as a fused kernel, the image conv: no runs
                continue
            run = -(-n // len(got))
            frames = [min(run, n - f0) for f0 in range(0, n, run)]
            assert len(frames) == len(got), (c["name"], got, frames)
            for name, f in zip(got, frames):
                assert net.conv_kernels(i, f, h, w, CUS) == [name], (c["name"], f, got)
                p = net.conv_plan(i, f, h, w, CUS)
                assert (p["bm"], p["bn"], p["small"]) == tile_of(name), (c["name"], f, name, p)
            for fewer in range(1, len(got)):
                size = -(-n // fewer)
                last = n - (-(-n // size) - 1) * size
                assert any(len(net.conv_kernels(i, f, h, w, CUS)) > 1 for f in (size, last)), (c["name"], fewer)
            if len(got) > 1:
                several.append(c["name"])
        assert several == (["conv1_2"] if n == FRAME_RUN_BATCH else [])
        if small:
            assert any(k.startswith("conv3s_kernel<") for i in range(len(net.convs()))
                       for k in net.conv_kernels(i, n, h, w, CUS))
    finally:
        net.close()


def test_conv_kernels_arguments(host):
    net = Net(host, BODY_25)
    try:
        n = len(net.convs())
        for args in ((-1, 1, 368, 656, CUS), (n, 1, 368, 656, CUS), (0, 0, 368, 656, CUS), (0, 1, 368, 656, 0)):
            with pytest.raises(Exception):
                net.conv_kernels(*args)
    finally:
        net.close()
