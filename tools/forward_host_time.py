#!/usr/bin/env python3
"""dev: host time of a net forward that is only enqueued (no wait for the GPU).

    python tools/forward_host_time.py [--frames 1] [--size 368 656] [--forwards 200] [--no-small]

BODY_25 with random weights, small-batch mode on by default (the 1-8 frame mode, where the host
path of a forward weighs most).  After a warm-up, times every `net.forward` call on its own with
no synchronisation inside the timed span, in two ways:

  free:    the forwards back to back, one sync at the end.  Once the stream's queue is full a
           call also waits for the GPU, so this figure is bounded below by the GPU time per forward;
  drained: a sync (untimed) after every forward, so each call enqueues into an empty queue: the
           host cost of a forward alone.

Prints one JSON line: median, quartiles and min of both, in microseconds.  Compare two builds by
running it once with OPK_LIB_PATH set to the other library.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from openpose_amd import _lib, synth                                  # noqa: E402
from openpose_amd.api import Context, Net                             # noqa: E402


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "q1_us": round(q[0], 2), "q3_us": round(q[2], 2),
            "min_us": round(min(us), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1)
    ap.add_argument("--size", type=int, nargs=2, default=[368, 656], metavar=("H", "W"))
    ap.add_argument("--forwards", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-small", action="store_true", help="leave the small-batch mode off")
    a = ap.parse_args()
    h, w = a.size
    ctx = Context(0)
    net = Net(ctx, "builtin:BODY_25")
    net.set_params(synth.he_weights(net.convs(), seed=0, out_scale=0.02))
    net.set_small_batch(not a.no_small)
    x = torch.from_numpy(np.random.default_rng(0).uniform(-0.5, 0.5, (a.frames, 3, h, w)).astype(np.float32)).cuda()
    out = {"lib": os.path.basename(_lib.LIB_PATH), "frames": a.frames, "size": [h, w], "small_batch": not a.no_small,
           "forwards": a.forwards}
    for mode in ("free", "drained"):
        for _ in range(a.warmup):
            net.forward(x)
        ctx.sync()
        us = []
        for _ in range(a.forwards):
            t0 = time.perf_counter()
            net.forward(x)
            us.append((time.perf_counter() - t0) * 1e6)
            if mode == "drained":
                ctx.sync()
        ctx.sync()
        out[mode] = stats(us)
    net.close()
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
