"""Record which kernel instantiation runs every conv: one forward per case of
tests/conv_dispatch_cases.py under LAUNCH_LOG=1, the (layer, kernel) pairs of its launch log written
to a JSON table.

    python tools/record_conv_dispatch.py OUT.json [--only SUBSTRING]

tests/golden/conv_dispatch_parent.json is this tool's output at the commit before the host-side
conv planner (conv_plan.cpp); tests/test_conv_dispatch.py holds Net.conv_kernels against it.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from openpose_amd.api import PRECISION_SPLIT, Context, Net, dev_switches   # noqa: E402
from tests.conv_dispatch_cases import cases, graph_of, model_path           # noqa: E402
from tests.launch_check import random_params                                # noqa: E402


def record(ctx, c, params):
    n, h, w = c["shape"]
    x = torch.zeros((n, 3, h, w), device="cuda")
    with model_path(c["model"]) as path, dev_switches(LAUNCH_LOG=1, **c["switches"]):
        net = Net(ctx, path)
        try:
            net.set_params(params)
            if c["split"]:
                net.set_precision(PRECISION_SPLIT)
            if c["small"]:
                net.set_small_batch(True)
            net.forward(x)
            ctx.sync()
            return [list(e) for e in net.launch_log()]
        finally:
            net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--only", default=None, help="cases whose name contains this")
    a = ap.parse_args()
    ctx = Context(0)
    table = dict(cus=torch.cuda.get_device_properties(0).multi_processor_count, cases=[])
    params = {}
    for c in cases():
        if a.only and a.only not in c["name"]:
            continue
        if c["model"] not in params:
            params[c["model"]] = random_params(graph_of(c["model"]), 7)
        log = record(ctx, c, params[c["model"]])
        assert log and np.all([len(e) == 2 for e in log]), c["name"]
        table["cases"].append(dict(c, log=log))
        print("%-60s %3d launches" % (c["name"], len(log)), flush=True)
    with open(a.out, "w") as f:
        json.dump(table, f, indent=0)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
