"""What rotating and flipping the frames costs: the permutation kernels alone against a device copy
of the same bytes, and the raw-frame pipeline with and without the stage.

    python tools/orient_bench.py --out profiles/orient/orient.json

(1) The kernels.  128 frames of 1280x720, BGR and NV12, each of the 8 orientations under both
    mappings (ORIENT_TILE: 1 the dword kernels, 0 the plain one), and in the same rounds a
    device-to-device copy of the frames' bytes -- what a perfect permutation must move, so the
    yardstick.  A round is one pair of HIP events around `--launches` back-to-back calls of one
    variant, divided by their number; `--repeats` rounds after a warm-up, the variants alternating,
    medians and the min-max spread.  gbs = 2 x the frames' bytes (read and written) over the median.
(2) The pose pipeline step (submit i + 1, collect i) on the same BGR frames, pose only: without the
    stage, with (180, 0) and with (90, 0), alternating.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import body25                                    # noqa: E402
from openpose_amd import api, synth                          # noqa: E402

SIZE = (1280, 720)
NET_H = 368
MAPPINGS = {"tiled": 1, "plain": 0}   # the ORIENT_TILE switch
CASES = [(r, f) for r in (0, 90, 180, 270) for f in (0, 1)]


def _summary(ms, nbytes):
    med = statistics.median(ms)
    return dict(rounds_ms=ms, median_ms=med, min_ms=min(ms), max_ms=max(ms), gbs=2 * nbytes / med / 1e6)


def _timed(ctx, fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.sync()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    ctx.sync()
    return a.elapsed_time(b) / launches


def _planes(frames):
    return frames.planes if isinstance(frames, api.Frames) else [frames]


def kernels(ctx, n, repeats, launches):
    g = torch.Generator().manual_seed(1)
    bgr = torch.randint(0, 256, (n, SIZE[1], SIZE[0], 3), dtype=torch.uint8, generator=g).cuda()
    sources = {"bgr": bgr, "nv12": api.Frames.from_bgr(ctx, bgr, "nv12")}
    res = dict(frames=n, launches_per_round=launches)
    for fmt, src in sources.items():
        nbytes = sum(p.numel() for p in _planes(src))
        copies = [torch.empty_like(p) for p in _planes(src)]

        def device_copy():
            for d, s in zip(copies, _planes(src)):
                d.copy_(s)
        calls = {"device_copy": device_copy}
        for rotate, flip in CASES:
            out = ctx.orient_frames(src, rotate, flip)            # the destination, reused
            kept = {}
            for m, switch in MAPPINGS.items():
                def call(rotate=rotate, flip=flip, out=out, switch=switch):
                    with api.dev_switches(ORIENT_TILE=switch):
                        ctx.orient_frames(src, rotate, flip, out=out)
                call()                                            # warm-up, and the two must agree
                ctx.sync()
                kept[m] = [p.clone() for p in _planes(out)]
                calls["%d_%d_%s" % (rotate, flip, m)] = call
            assert all(torch.equal(a, b) for a, b in zip(kept["tiled"], kept["plain"])), (fmt, rotate, flip)
        device_copy()
        rows = {name: [] for name in calls}
        for _ in range(repeats):
            for name, call in calls.items():
                rows[name].append(_timed(ctx, call, launches))
        r = {name: _summary(ms, nbytes) for name, ms in rows.items()}
        for name in r:
            r[name]["times_device_copy"] = r[name]["median_ms"] / r["device_copy"]["median_ms"]
        r["frame_bytes"] = nbytes
        res[fmt] = r
    return res


def _step(ctx, pose, bufs, batches):
    ctx.sync()
    t0 = time.perf_counter()
    pose.submit_frames(bufs[0])
    for b in range(1, batches):
        pose.submit_frames(bufs[b & 1])   # batch b - 1's frames stay until its collect
        pose.collect()
    pose.collect()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / batches


def _overlay(size, n):
    _, net_sizes = api.scale_and_size(size, (-1, NET_H))
    W, H = net_sizes[0]
    distinct = [synth.overlay(1, H // 8, W // 8, seed=s) for s in range(8)]
    return torch.from_numpy(np.stack([distinct[f % 8] for f in range(n)])).cuda()


def pipeline(ctx, n, repeats, batches):
    g = torch.Generator().manual_seed(1)
    bufs = [torch.randint(0, 256, (n, SIZE[1], SIZE[0], 3), dtype=torch.uint8, generator=g).cuda()
            for _ in range(2)]
    net = api.Net(ctx, "builtin:BODY_25")
    net.set_params(synth.he_weights(body25.layers(), seed=3, out_scale=0.02))
    pose = api.PoseExtractor(ctx, net)
    pose.set_input((-1, NET_H))
    # the overlay has the net output's shape, which follows the oriented frame size
    settings = {"no_stage": ((0, 0), _overlay(SIZE, n)), "rotate_180": ((180, 0), _overlay(SIZE, n)),
                "rotate_90": ((90, 0), _overlay(SIZE[::-1], n))}
    rows = {k: [] for k in settings}
    for r in range(repeats + 1):                     # round 0 warms every setting up
        for name, (orientation, overlay) in settings.items():
            pose.set_orientation(*orientation)
            pose.set_overlay(overlay)
            ms = _step(ctx, pose, bufs, batches)
            if r:
                rows[name].append(ms)
    out = {k: dict(ms_per_batch=v, median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v),
                   frames_per_s=n / statistics.median(v) * 1e3) for k, v in rows.items()}
    pose.close()
    net.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = api.Context(0)
    res = dict(frames=a.frames, size=list(SIZE), repeats=a.repeats, batches=a.batches,
               device=torch.cuda.get_device_name(0), library=os.path.basename(api._lib.LIB_PATH))
    res["kernels"] = kernels(ctx, a.frames, a.repeats, a.launches)
    res["pipeline"] = pipeline(ctx, a.frames, a.repeats, a.batches)
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
