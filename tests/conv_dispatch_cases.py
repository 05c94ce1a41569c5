"""The forwards whose conv dispatch tests/golden/conv_dispatch_parent.json records: which kernel
instantiation runs every conv of a graph at a shape, precision, small-batch flag and switch set.

Shared by tools/record_conv_dispatch.py (one forward per case on the GPU, the launch log written
down) and tests/test_conv_dispatch.py (Net.conv_kernels on a host-only context against the table).
The graphs are the builders of tests/test_gpu_launch_matrix.py and tests/test_gpu_net.py.
"""
import contextlib
import os
import tempfile

from tests import prototxt
from tests.test_gpu_launch_matrix import AB_SWITCHES, front_graph, variants_graph
from tests.test_gpu_net import conv, cpm_stage_graph

BODY_25 = "builtin:BODY_25"


def narrow_graph():
    """Case d of tests/test_gpu_launch_matrix.py (built inline there)."""
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", 64, 3, "prelu")
    L += conv("c3", "c2", 128, 3, "relu") + conv("c4", "c3", 96, 3, "prelu") + conv("c5", "c4", 52, 1)
    L.append(dict(name="net_output", type="Concat", bottom=["c5"], top=["net_output"]))
    return L


GRAPHS = {"front": front_graph, "narrow": narrow_graph, "variants": variants_graph,
          "cpm7": lambda: cpm_stage_graph(True)}

# conv1_2 of BODY_25 at 368 x 656 in split precision (no conv1 fusion) plans eight 82-column strips
# of the persistent 512 / 688 tile: frames * 8 * 370 * 84 + 512 + 2 * 85 positions, below 2^24 up
# to 67 frames.  68 is the smallest batch whose conv1_2 runs as two frame runs.
FRAME_RUN_BATCH = 68
assert 67 * 8 * 370 * 84 + 512 + 2 * 85 < 1 << 24 <= 68 * 8 * 370 * 84 + 512 + 2 * 85

# the decision switches flipped one at a time (asked again of a net planned under them)
FLIPS = [dict(CONV3W8_64=0), dict(CONV3_PERSIST=0), dict(CONV3_W16=0), dict(CONV3_SMALL=0)]


def case(model, shape, split=False, small=False, **switches):
    name = "%s %dx%dx%d %s%s" % ((model.split(":")[-1], ) + tuple(shape) +
                                ("split" if split else "fp16", " small" if small else ""))
    for k in sorted(switches):
        name += " %s=%d" % (k, switches[k])
    return dict(name=name, model=model, shape=list(shape), split=split, small=small, switches=switches)


def cases():
    out = []
    for shape in ((130, 368, 656), (1, 368, 656)):
        for split in (False, True):
            for small in (False, True):
                out.append(case(BODY_25, shape, split, small))
    for shape in ((2, 64, 96), (1, 50, 90), (1, 272, 480)):
        for split in (False, True):
            out.append(case(BODY_25, shape, split))
    for split in (False, True):   # (the small-batch flag at the GPU test's shape)
        out.append(case(BODY_25, (2, 64, 96), split, True))
    for name in ("a", "b", "w8_64_off"):
        out.append(case("front", (4, 184, 328), **AB_SWITCHES[name]))
    out.append(case("front", (4, 183, 327)))                       # c
    out.append(case("front", (1, 16, 36), CONV1_FUSED=0))          # (the GPU test's small graph)
    for split in (False, True):
        out.append(case("narrow", (48, 254, 14), split))           # d
    out.append(case("variants", (2, 256, 386)))                    # e
    out.append(case("variants", (2, 256, 386), CONV3_W16=0, CONV1_TILE=0))
    for split in (False, True):
        out.append(case("cpm7", (2, 64, 96), split))               # g
    out.append(case(BODY_25, (FRAME_RUN_BATCH, 368, 656), True))   # conv1_2 in two frame runs
    out.append(case("front", (4, 184, 328), True, CONV1_FUSED=0))  # (the flips' split base)
    for flip in FLIPS:
        out.append(case("variants", (2, 256, 386), **flip))
        for split in (False, True):
            out.append(case("front", (4, 184, 328), split, CONV1_FUSED=0, **flip))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


@contextlib.contextmanager
def model_path(model):
    """The prototxt path (or "builtin:...") Net takes for a case's model."""
    if model.startswith("builtin:"):
        yield model
        return
    with tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False) as f:
        f.write(prototxt.emit(GRAPHS[model]()))
    try:
        yield f.name
    finally:
        os.unlink(f.name)


def graph_of(model):
    """The parsed layer list of a case's model (names, for random parameters)."""
    if model.startswith("builtin:"):
        from oracle import body25
        return body25.layers()
    return prototxt.parse(prototxt.emit(GRAPHS[model]()))
