"""The frame warp on NV12 frames against BGR frames, and the pose-only pipeline step on both.

    python tools/yuv_input_bench.py --out profiles/yuv_input/yuv_input.json

Workload: 130 frames of 1280x720 -> the 656x368 net input (scale and size from
ScaleAndSizeExtractor), the warp alone:
  (a) bgr        cvmat_to_input on BGR frames -- the kernel every earlier commit has;
  (b) nv12       cvmat_to_input on NV12 frames, converted inside the warp;
  (c) nv12_2pass opk_frames_to_bgr into a BGR batch, then (a) on it -- the plain chain (b) replaces.
The three alternate in one process after one warm-up round, `--repeats` rounds each; a round is
`--iters` calls ended by one stream synchronisation, timed with the host clock (a window of tens of
milliseconds).  Then the pose-only pipeline step (submit i + 1, collect i; seeded BODY_25 weights,
no overlay) on BGR and on NV12 frames, alternating likewise.  Reported: every round's
milliseconds per batch, the median, and the bytes each variant moves per frame.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import body25                                    # noqa: E402
from openpose_amd import api, synth                          # noqa: E402

SIZE = (1280, 720)


def _planes(n, seed):
    g = torch.Generator().manual_seed(seed)
    w, h = SIZE
    y = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, generator=g).cuda()
    uv = torch.randint(0, 256, (n, h // 2, w), dtype=torch.uint8, generator=g).cuda()
    return y, uv


def _timed(ctx, fn, iters):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / iters


def _rounds(ctx, variants, repeats, iters):
    """{name: [ms per call of every round]}, the variants alternating; one untimed round first."""
    for fn in variants.values():
        _timed(ctx, fn, 1)
    out = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            out[k].append(_timed(ctx, fn, iters))
    return out


def _summary(rounds, n):
    res = {}
    for k, ms in rounds.items():
        med = statistics.median(ms)
        res[k] = dict(ms_per_batch=ms, median_ms=med, frames_per_s=n / med * 1e3)
    return res


def warp(ctx, n, repeats, iters):
    scales, sizes = api.scale_and_size(SIZE, (-1, 368))
    net_w, net_h = sizes[0]
    y, uv = _planes(n, 1)
    nv12 = api.Frames.nv12(y, uv)
    bgr = nv12.to_bgr(ctx)
    scratch = torch.empty_like(bgr)
    out = torch.empty((n, 3, net_h, net_w), dtype=torch.float32, device="cuda")
    want = torch.empty_like(out)
    ctx.cvmat_to_input(want, bgr, scales[0])
    ctx.cvmat_to_input(out, nv12, scales[0])
    ctx.sync()
    assert torch.equal(out, want), "the fused warp differs from the two-pass chain"

    def two_pass():
        nv12.to_bgr(ctx, scratch)
        ctx.cvmat_to_input(out, scratch, scales[0])

    variants = {"bgr": lambda: ctx.cvmat_to_input(out, bgr, scales[0]),
                "nv12": lambda: ctx.cvmat_to_input(out, nv12, scales[0]),
                "nv12_2pass": two_pass}
    with api.launch_log() as log:
        for fn in variants.values():
            fn()
    res = _summary(_rounds(ctx, variants, repeats, iters), n)
    src = SIZE[0] * SIZE[1]
    dst = 3 * net_w * net_h * 4
    # bytes per frame if every source byte is read once: an upper bound on what the format can gain
    res["bytes_per_frame"] = {"bgr": 3 * src + dst, "nv12": src * 3 // 2 + dst,
                              "nv12_2pass": src * 3 // 2 + 3 * src + 3 * src + dst}
    res["kernels"] = [k for _, k in log]
    res["net_input"] = [net_w, net_h]
    return res


def pose_step(ctx, n, repeats, batches):
    net = api.Net(ctx, "builtin:BODY_25")
    net.set_params(synth.he_weights(body25.layers(), seed=3, out_scale=0.02))
    pose = api.PoseExtractor(ctx, net)
    pose.set_input((-1, 368))
    sets = {}
    for b in range(2):   # two buffers: batch b - 1's frames stay until its collect
        y, uv = _planes(n, 10 + b)
        f = api.Frames.nv12(y, uv)
        sets.setdefault("nv12", []).append(f)
        sets.setdefault("bgr", []).append(f.to_bgr(ctx))

    def loop(bufs):
        def run():
            pose.submit_frames(bufs[0])
            for b in range(1, batches):
                pose.submit_frames(bufs[b & 1])
                pose.collect()
            pose.collect()
        return run

    rounds = _rounds(ctx, {k: loop(v) for k, v in sets.items()}, repeats, 1)
    res = _summary({k: [ms / batches for ms in v] for k, v in rounds.items()}, n)
    pose.close()
    net.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=130)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--no-pose", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = api.Context(0)
    res = dict(frames=a.frames, size=list(SIZE), repeats=a.repeats, iters=a.iters,
               device=torch.cuda.get_device_name(0), warp=warp(ctx, a.frames, a.repeats, a.iters))
    if not a.no_pose:
        res["pose_step"] = dict(batches=a.batches, **pose_step(ctx, a.frames, a.repeats, a.batches))
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
