"""Per-launch checker for nets under a per-layer precision schedule (Net.set_precision_schedule):
tests/launch_check.py's check with every launch referenced to its OWN precision.

check_schedule() takes a net after a forward under LAUNCH_LOG=1 and the schedule {conv name:
precision} it ran, and compares, element by element:

  * an fp16 unit with the fp16-storage emulation (oracle/fp16.py) fed the HI plane of the GPU's own
    input blob (blob_planes) -- an fp16 layer reads the hi image of whatever it reads, a split
    writer's lo twin is not its input -- its stored hi plane within 2 ulp16 + C_ACC S (C_ACC_CHAINED
    for a fused unit);
  * a split unit with the float64 conv (oracle/split.py) of hi + lo of the input blob -- after an
    fp16 writer the lo plane is zero, which the hi-only kernels rely on and the last check below
    asserts -- hi + lo of its output within C_SPLIT S: a hi-only kernel that dropped the x_hi w_lo
    product is ~2^-11 S off;
  * a fused unit's convs share one precision (the planner fuses nothing else): asserted;
  * heads' fp32 slices of net_output, check_concat_slices and the stand-alone pools exactly, as
    launch_check.check_launches;
  * for every materialised conv, pool and concat blob: the lo plane is exactly zero on the channels
    whose writer is fp16 (a pool: the writer of its input) -- a stale lo under an fp16 writer would
    be read by the next three-product kernel.

The net needs blob(name, (f, 1)), blob_planes(name, (f, 1)) -> (hi, lo, has_lo) and launch_log().
"""
import collections

import numpy as np

from oracle import fp16 as emu
from oracle import split as sp
from tests.launch_check import (C_ACC, C_ACC_CHAINED, C_SPLIT, Row, _compare, check_concat_slices)

FP16, SPLIT = 0, 1


def _materialised(net, name, f):
    try:
        return net.blob_planes(name, (f, 1))
    except Exception as e:   # kept on chip by a fused kernel
        if "kept on chip" in str(e):
            return None
        raise


def check_lo_zero(net, graph, schedule, frames):
    """The lo plane of every blob is exactly zero on the channels an fp16 conv wrote (a pool's
    output: where its input's writer is fp16).  Returns the number of (blob, writer) slices seen."""
    chans = {l["top"][0]: l["num_output"] for l in graph if l["type"] == "Convolution"}
    writer = {l["top"][0]: l["name"] for l in graph if l["type"] == "Convolution"}
    for l in graph:
        if l["type"] == "Pooling":
            writer[l["top"][0]] = writer[l["bottom"][0]]
            chans[l["top"][0]] = chans[l["bottom"][0]]
    slices = []   # (blob, first channel, channels, writing conv)
    for l in graph:
        if l["type"] in ("Convolution", "Pooling"):
            slices.append((l["top"][0], 0, chans[l["top"][0]], writer[l["top"][0]]))
        elif l["type"] == "Concat" and l["top"][0] != "net_output":
            off = 0
            for b in l["bottom"]:
                slices.append((l["top"][0], off, chans[b], writer[b]))
                off += chans[b]
    seen = 0
    for blob, off, ch, conv in slices:
        if schedule[conv] != FP16:
            continue
        for f in frames:
            planes = _materialised(net, blob, f)
            if planes is None:
                continue
            lo = planes[1][:, off:off + ch]
            bad = lo != 0
            if bad.any():
                i = tuple(int(v) for v in np.unravel_index(np.argmax(bad), bad.shape))
                raise AssertionError("%s (lo plane) channels [%d, %d) written by the fp16 conv %s, frame "
                                     "%d: %d of %d lo elements are not zero; first at %s: lo %r tol 0"
                                     % (blob, off, off + ch, conv, f, int(bad.sum()), bad.size, i,
                                        float(lo[i])))
            seen += f == frames[0]
    return seen


def check_schedule(net, graph, params, x, frames, schedule, log=None):
    """schedule: {conv name: FP16 / SPLIT} of the forward the net just ran.  Returns [Row] as
    check_launches (fp16 units' rows carry ulp16); raises AssertionError naming layer, kernel,
    frame, element, GPU value, reference and bound."""
    log = net.launch_log() if log is None else log
    kernels = collections.OrderedDict()
    pool_kernels = []
    for layer, kernel in log:
        if layer == "pool":
            pool_kernels.append(kernel)
        elif kernel not in kernels.setdefault(layer, []):
            kernels[layer].append(kernel)
    rows, units, unit_split = [], {}, {}
    for layer, ks in kernels.items():
        kernel = " ".join(ks)
        u = units[layer] = emu.unit_from_launch(graph, layer)
        precs = {schedule[c["name"]] for c in u["convs"]}
        assert len(precs) == 1, "%s (%s): a fused unit of mixed precisions %r" % (layer, kernel, precs)
        split = unit_split[layer] = precs.pop() == SPLIT
        worst = (0.0, 0.0, 0.0)
        for f in frames:
            if u["input"] == "image":
                xin = x[f:f + 1]
            elif split:
                xin = net.blob(u["input"], (f, 1))            # hi + lo
            else:
                xin = net.blob_planes(u["input"], (f, 1))[0]  # the hi image
            if split:
                ref, tol = sp.unit(u, xin, params, C_SPLIT)
                got = net.blob(u["output"], (f, 1))
            else:
                ref, tol = emu.unit(u, xin, params, C_ACC_CHAINED if len(u["convs"]) > 1 else C_ACC)
                got = net.blob_planes(u["output"], (f, 1))[0]
            w = _compare("split bound" if split else "bound", layer, kernel, f, got, ref, tol, split)
            worst = tuple(max(a, b) for a, b in zip(worst, w))
        rows.append(Row(layer, kernel, *worst))

    out = [l for l in graph if l["type"] == "Concat" and l["top"][0] == "net_output"]
    if out:
        off = 0
        chans = {l["top"][0]: l["num_output"] for l in graph if l["type"] == "Convolution"}
        for b in out[0]["bottom"]:
            head = [lay for lay, u in units.items() if u["output"] == b and u["pool"] is None]
            assert len(head) == 1, (b, head)
            u, split = units[head[0]], unit_split[head[0]]
            if u["fp32_output"]:
                for f in frames:
                    if split:
                        ref, tol = sp.unit(u, net.blob(u["input"], (f, 1)), params, C_SPLIT)
                    else:
                        ref, tol = emu.unit(u, net.blob_planes(u["input"], (f, 1))[0], params,
                                            C_ACC_CHAINED if len(u["convs"]) > 1 else C_ACC)
                    got = net.blob("net_output", (f, 1))[:, off:off + ref.shape[1]]
                    _compare(("split bound" if split else "bound") + " (net_output slice)", head[0],
                             " ".join(kernels[head[0]]), f, got, ref, tol, split)
            off += chans[b]
        assert off == net.blob("net_output", (frames[0], 1)).shape[1], off

    check_concat_slices(net, graph, frames)

    fused = {u["pool"]["name"] for u in units.values() if u["pool"] is not None}
    alone = [l for l in graph if l["type"] == "Pooling" and l["name"] not in fused]
    assert len(alone) == len(pool_kernels), ("pool launches", [l["name"] for l in alone], pool_kernels)
    for l, kernel in zip(alone, pool_kernels):
        amax = 0.0
        for f in frames:
            xin = net.blob(l["bottom"][0], (f, 1))
            got = net.blob(l["top"][0], (f, 1))
            ref = sp._maxpool64(xin.astype(np.float64), l["kernel_size"], l["stride"])
            assert got.shape == ref.shape, (l["name"], got.shape, ref.shape)
            bad = got.astype(np.float64) != ref
            if bad.any():
                i = np.unravel_index(np.argmax(bad), bad.shape)
                raise AssertionError("%s (%s) frame %d: %d of %d pooled elements differ from the max "
                                     "of the input blob; first at %s: gpu %r ref %r tol 0"
                                     % (l["name"], kernel, f, int(bad.sum()), bad.size, i,
                                        float(got[i]), float(ref[i])))
            amax = max(amax, float(np.abs(ref).max()))
        rows.append(Row(l["name"], kernel, 0.0, 0.0, amax))

    check_lo_zero(net, graph, schedule, frames)
    return rows
