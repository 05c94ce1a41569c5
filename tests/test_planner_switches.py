"""CPU: every planner switch of conv.h's list, one at a time, plans kernels that exist.

conv3_plan ends with a check of the plan's family and tile against the list of instantiations
(csrc/kernels/conv_tiles.h), so on a host-only context Net.conv_kernels returning for a conv proves
that a launch of it would find its kernel; a plan off the list raises "no instantiation of <name>".
Each switch is set to each value the planner distinguishes, over BODY_25 at one frame and at the
bench batch and one 7x7 net (tests/cpm_graphs.py) at one crop, in fp16, split and an fp16-trunk /
split-stages schedule, small-batch mode off and on.

EXPECTED_HOLES lists, by name, the cases whose plan is a tile nobody instantiated -- holes the
check made visible, kept as planner errors (no instantiation is added for a dev switch).  There
are none today.
"""
import pytest

from openpose_amd.api import PRECISION_FP16, PRECISION_SPLIT, Context, Net, OpkError, dev_switches
from tests import cpm_graphs

CUS = 256
SWITCHES = [("CONV3_SMALL", 0), ("CONV3_W16", 0), ("CONV3_PERSIST", 0),
            ("CONV1_TILE", 0), ("CONV1_TILE", 1), ("CONV1_TILE", 2), ("CONV1_N64W16", 1),
            ("CONV3W8_64", 0), ("SPLIT_W8", 0), ("CONV3W8N", 0), ("CONV3W", 0),
            ("CONV3W8", 0), ("CONV3W8", 2), ("CONV3W8", 3), ("SPLIT_XHI", 0), ("SPLIT_XHI_W8", 0)]
NETS = [("builtin:BODY_25", (1, 368, 656)), ("builtin:BODY_25", (130, 368, 656)),
        ("builtin:FACE", (1, 368, 368))]
PRECISIONS = ["fp16", "split", "fp16-trunk"]

# (switch=value, model, frames, precision, small-batch) -> kernel names the planner refuses
EXPECTED_HOLES = {}


@pytest.fixture(scope="module")
def host():
    c = Context.host_only()
    yield c
    c.close()


@pytest.fixture(scope="module")
def nets(host):
    assert "builtin:FACE" in cpm_graphs.GRAPHS
    made = {}
    for model, _ in NETS:
        for prec in PRECISIONS:
            if (model, prec) in made:
                continue
            n = made[(model, prec)] = Net(host, model)
            if prec == "split":
                n.set_precision(PRECISION_SPLIT)
            elif prec == "fp16-trunk":
                n.set_precision_schedule(
                    lambda c: PRECISION_SPLIT if c["name"].startswith("Mconv") else PRECISION_FP16)
    yield made
    for n in made.values():
        n.close()


@pytest.mark.parametrize("switch,value", SWITCHES, ids=["%s=%d" % s for s in SWITCHES])
def test_every_planned_kernel_exists(nets, switch, value):
    holes, planned = {}, 0
    with dev_switches(**{switch: value}):
        for model, shape in NETS:
            for prec in PRECISIONS:
                net = nets[(model, prec)]
                for small in (False, True):
                    net.set_small_batch(small)
                    case = ("%s=%d" % (switch, value), model, shape[0], prec, small)
                    for i, c in enumerate(net.convs()):
                        try:
                            planned += len(net.conv_kernels(i, *shape, CUS))
                        except OpkError as e:
                            assert "no instantiation of " in str(e), (case, c["name"], str(e))
                            holes.setdefault(case, set()).add(str(e).split("no instantiation of ")[1])
                    net.set_small_batch(False)
    assert planned > 0
    want = {k: v for k, v in EXPECTED_HOLES.items() if k[0] == "%s=%d" % (switch, value)}
    assert holes == want
