"""Per-layer-class kernel time and launch gaps of one BODY_25 forward of 368 x 656 frames (one frame
unless a frame count is given), or of another net and size (classes by kernel size: 7x7, 3x3, 1x1).

Run mode, under a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
        python tools/small_batch_trace.py run {fp16|split} {off|on} DIR/launches.json [frames [model HxW]]

forwards the batch 30 times and writes the launch log (layer, kernel) of a forward.  Summary mode

    python tools/small_batch_trace.py summary DIR/.../run_kernel_trace.csv DIR/launches.json

takes the last forward of the trace, labels its launches with the log's layers (same order) and
prints the kernel time per layer class, the span of the forward and the sum of the gaps between
consecutive kernels, as one JSON line.
"""
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def layer_class(layer):
    if layer == "pool":
        return "pools"
    first = layer.split("+")[0]
    if first.startswith(("conv1_", "conv2_")):
        return "conv1_* conv2_* (368x656, 184x328)"
    if first.startswith("conv3_"):
        return "conv3_* (92x164)"
    if first.startswith("conv4_"):
        return "conv4_* (46x82)"
    if first.startswith(("Mconv6", "Mconv7")):
        return "stage heads 1x1 (Mconv6+7)"
    return "stage 3x3 (Mconv1-5, 46x82)"


def size_class(kernel_sizes, layer):
    """Another model than BODY_25: the launches by kernel size (the first conv of a fused unit)."""
    if layer == "pool":
        return "pools"
    first = layer.split("+")[0]
    if first == "conv1_1":
        return "image conv"
    return "%dx%d convs" % (kernel_sizes[first], kernel_sizes[first])


def run(precision, flag, out, frames=1, model="builtin:BODY_25", hw=(368, 656)):
    import numpy as np
    import torch
    from openpose_amd import synth
    from openpose_amd.api import PRECISION_SPLIT, Context, Net, dev_switches
    if not torch.cuda.is_available():
        sys.exit("small_batch_trace: no GPU")
    ctx = Context(0)
    net = Net(ctx, model)
    net.set_params(synth.he_weights(net.convs(), seed=0, out_scale=1.0))
    if precision == "split":
        net.set_precision(PRECISION_SPLIT)
    if flag == "on":
        net.set_small_batch(True)
    x = torch.from_numpy(np.random.default_rng(1).uniform(-0.5, 0.5, (frames, 3) + tuple(hw)).astype(np.float32)).cuda()
    with dev_switches(LAUNCH_LOG=1):
        net.forward(x)
        log = net.launch_log()
    for _ in range(30):
        net.forward(x)
    torch.cuda.synchronize()
    if model != "builtin:BODY_25":   # (summary: classes by kernel size)
        log = {"log": log, "kernel_size": {c["name"]: c["kernel_size"] for c in net.convs()}}
    with open(out, "w") as f:
        json.dump(log, f)
    net.close()
    ctx.close()


def summary(trace, launches):
    log = json.load(open(launches))
    classify = layer_class
    if isinstance(log, dict):
        sizes, log = log["kernel_size"], log["log"]
        classify = lambda layer: size_class(sizes, layer)
    rows = [r for r in csv.DictReader(open(trace))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    first = log[0][1].split("<")[0]
    starts = [i for i, r in enumerate(rows) if first in r["Kernel_Name"]]
    seg = rows[starts[-1]:starts[-1] + len(log)]
    assert len(seg) == len(log), (len(seg), len(log))
    classes, kernels = {}, {}
    for (layer, kernel), r in zip(log, seg):
        assert kernel.split("<")[0] in r["Kernel_Name"], (kernel, r["Kernel_Name"])
        d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        c = classes.setdefault(classify(layer), [0, 0.0])
        c[0] += 1
        c[1] += d
        k = kernels.setdefault(kernel, [0, 0.0])
        k[0] += 1
        k[1] += d
    busy = sum(v[1] for v in classes.values())
    span = (int(seg[-1]["End_Timestamp"]) - int(seg[0]["Start_Timestamp"])) / 1e3
    gaps = sum(max(0, int(b["Start_Timestamp"]) - int(a["End_Timestamp"])) for a, b in zip(seg, seg[1:])) / 1e3
    print(json.dumps({"launches": len(seg), "span_us": round(span, 1), "kernels_us": round(busy, 1),
                      "gaps_us": round(gaps, 1),
                      "classes_us": {k: [v[0], round(v[1], 1)] for k, v in sorted(classes.items())},
                      "kernels_us_by_name": {k: [v[0], round(v[1], 1)] for k, v in sorted(kernels.items())}}))


if __name__ == "__main__":
    if len(sys.argv) in (5, 6) and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]) if len(sys.argv) == 6 else 1)
    elif len(sys.argv) == 8 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]), sys.argv[6],
            tuple(int(v) for v in sys.argv[7].split("x")))
    elif len(sys.argv) == 4 and sys.argv[1] == "summary":
        summary(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
