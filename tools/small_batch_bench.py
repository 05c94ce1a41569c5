"""Forward time of a net (BODY_25 by default) at the batch sizes an OpenPose worker runs (1 - 8 frames), with the
small-batch mode (Net.set_small_batch) off and on, in fp16 and split precision: HIP events around
each forward (opk_net_set_timing), milliseconds per forward.

    python tools/small_batch_bench.py --out result.json [--flag-off-only] [--repeats 3]
                                      [--warmup 20] [--steps 200]
                                      [--model builtin:FACE] [--shapes 1x368x368,2x368x368]

Shapes (default): N in {1, 2, 4, 8} at 368 x 656, and 1 x 368 x 368.  Every repeat runs all variants of all
shapes in turn (variants alternated), so drift hits them alike; the JSON holds every repeat of every
leg, their mean and their spread (max - min).  The library is the one openpose_amd loads
(OPK_LIB_PATH selects another build; --flag-off-only for one without the mode).  Needs a GPU: there
is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1, 368, 656), (2, 368, 656), (4, 368, 656), (8, 368, 656), (1, 368, 368)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--flag-off-only", action="store_true", help="a library without the mode")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--model", default="builtin:BODY_25", help="a builtin net or a prototxt path")
    ap.add_argument("--shapes", default=None, help="comma-separated NxHxW (default: the BODY_25 set)")
    a = ap.parse_args()
    assert a.warmup >= 20 and a.steps >= 200 and a.repeats >= 1, "at least 20 warm-up and 200 timed forwards"
    shapes = SHAPES if a.shapes is None else [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    assert all(len(s) == 3 and min(s) > 0 for s in shapes), "--shapes: NxHxW[,NxHxW...]"

    import torch
    if not torch.cuda.is_available():
        sys.exit("small_batch_bench: no GPU")
    from openpose_amd import _lib, synth
    from openpose_amd.api import PRECISION_FP16, PRECISION_SPLIT, Context, Net

    ctx = Context(0)
    variants = [("fp16", PRECISION_FP16, False), ("fp16", PRECISION_FP16, True),
                ("split", PRECISION_SPLIT, False), ("split", PRECISION_SPLIT, True)]
    if a.flag_off_only:
        variants = [v for v in variants if not v[2]]
    nets = {}
    params = None
    for prec_name, prec, small in variants:
        net = Net(ctx, a.model)
        if params is None:
            params = synth.he_weights(net.convs(), seed=0, out_scale=1.0)
        net.set_params(params)
        net.set_precision(prec)
        if small:
            net.set_small_batch(True)   # (a library without the symbol fails here)
            assert net.small_batch
        nets[(prec_name, small)] = net

    rng = np.random.default_rng(1)
    legs = {}
    for n, h, w in shapes:
        x = torch.from_numpy(rng.uniform(-0.5, 0.5, (n, 3, h, w)).astype(np.float32)).cuda()
        for _ in range(a.repeats):
            for key, net in nets.items():
                for _ in range(a.warmup):
                    net.forward(x)
                torch.cuda.synchronize()
                net.set_timing(True)
                for _ in range(a.steps):
                    net.forward(x)
                k, ms = net.read_timing()
                net.set_timing(False)
                assert k == a.steps, (k, a.steps)
                name = "%dx%dx%d %s %s" % (n, h, w, key[0], "on" if key[1] else "off")
                legs.setdefault(name, []).append(ms / k)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {"model": a.model, "library": os.path.relpath(os.path.realpath(_lib.LIB_PATH), root), "device": torch.cuda.get_device_name(0),
           "warmup": a.warmup, "steps": a.steps, "repeats": a.repeats, "legs": {}}
    for name, v in legs.items():
        res["legs"][name] = {"ms": [round(t, 4) for t in v], "mean_ms": round(float(np.mean(v)), 4),
                             "spread_ms": round(max(v) - min(v), 4)}
        print("%-28s %s  mean %.4f  spread %.4f" % (name, " ".join("%.4f" % t for t in v), np.mean(v),
                                                  max(v) - min(v)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    for net in nets.values():
        net.close()
    ctx.close()


if __name__ == "__main__":
    main()
