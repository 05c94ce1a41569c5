"""The batch render into NV12 / I420 frames against the BGR render, and opk_bgr_to_frames alone.

    python tools/yuv_output_bench.py --out profiles/yuv_output/yuv_output.json
    OPK_LIB_PATH=<the parent commit's libopk_hip.so> python tools/yuv_output_bench.py \
        --out profiles/yuv_output/parent_run1.json

Workload: 130 frames of 1280x720 with 20 people each as one POSE layer, drawn at the frames' size
(the copy route of the warp), both source formats:
  (a) bgr_out          render_frames into a BGR tensor -- the call every earlier commit has;
  (b) nv12_out, i420_out  render_frames into a Frames: converted in the store epilogue;
  (c) bgr_out+convert  (a), then opk_bgr_to_frames of its result -- the route (b) replaces;
  (d) convert          opk_bgr_to_frames alone, with its GB/s (bytes read + written) against the
                       measured streaming-read ceiling (opk_probe_peaks, what bench.py --full
                       reports) and against a device-to-device copy of the same BGR batch.
The variants alternate in one process after one warm-up round, `--repeats` rounds each; a round is
`--iters` calls ended by one stream synchronisation, timed with the host clock.  Reported: every
round's milliseconds per batch, the median, minimum and maximum.  A library without the frames-out
entry points (the parent commit's, loaded through OPK_LIB_PATH) runs (a) alone, as does
--bgr-only on any library: the BGR-out regression is (a) alone from two libraries -- the same
process on both sides, no other variant's buffers or cache traffic in between -- run several times
each, alternating; the spread of the parent's medians is the margin.
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

from openpose_amd import _lib, api                            # noqa: E402

SIZE = (1280, 720)


def _timed(ctx, fn, iters):
    ctx.sync()
    torch.cuda.synchronize()   # (the device copy runs on torch's stream)
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    ctx.sync()
    torch.cuda.synchronize()
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


def _summary(rounds):
    return {k: dict(ms_per_batch=[round(v, 4) for v in ms], median_ms=round(statistics.median(ms), 4),
                    min_ms=round(min(ms), 4), max_ms=round(max(ms), 4)) for k, ms in rounds.items()}


def _people_layer(n, people, seed):
    """`people` BODY_25 people per frame, in frame pixels: each one's 25 parts scattered over a
    160 x 280 box around a random centre (limbs of a person's size, people overlapping)."""
    w, h = SIZE
    g = np.random.default_rng(seed)
    kp = np.empty((n * people, 25, 3), np.float32)
    cx = g.uniform(100, w - 100, (n * people, 1))
    cy = g.uniform(150, h - 150, (n * people, 1))
    kp[..., 0] = cx + g.uniform(-80, 80, (n * people, 25))
    kp[..., 1] = cy + g.uniform(-140, 140, (n * people, 25))
    kp[..., 2] = 1.0
    return api.RenderLayer(api.LAYER_POSE, torch.from_numpy(kp.astype(np.float32)).cuda(),
                           [people] * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=130)
    ap.add_argument("--people", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--bgr-only", action="store_true",
                    help="(a) alone, whatever the library has: the like-for-like regression run")
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = api.Context(0)
    n, (w, h) = a.frames, SIZE
    has_out = hasattr(_lib.load(), "opk_render_frames_to") and not a.bgr_only
    g = torch.Generator().manual_seed(1)
    bgr = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g).cuda()
    layers = [_people_layer(n, a.people, 7)]
    out_bgr = torch.empty_like(bgr)
    res = dict(frames=n, size=list(SIZE), people=a.people, repeats=a.repeats, iters=a.iters,
               device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH), frames_out=has_out)
    sources = {"bgr": bgr}
    if has_out:
        sources["nv12"] = api.Frames.from_bgr(ctx, bgr, "nv12")
    for sname, src in sources.items():
        variants = {"bgr_out": lambda src=src: ctx.render_frames(src, layers, out=out_bgr)}
        if has_out:
            dst = {f: api.Frames.empty(f, n, h, w) for f in ("nv12", "i420")}
            for f in dst:
                variants[f + "_out"] = lambda src=src, f=f: ctx.render_frames(src, layers, out=dst[f])

            def two_pass(src=src):
                ctx.render_frames(src, layers, out=out_bgr)
                api.Frames.from_bgr(ctx, out_bgr, None, out=dst["nv12"])

            variants["bgr_out+convert"] = two_pass
            # the fused result is the two-pass chain's, bit for bit
            variants["nv12_out"]()
            fused = [p.clone() for p in dst["nv12"].planes]
            two_pass()
            ctx.sync()
            assert all(torch.equal(x, y) for x, y in zip(fused, dst["nv12"].planes))
        with api.launch_log() as log:
            for fn in variants.values():
                fn()
        res["render_from_" + sname] = dict(kernels=[k for _, k in log],
                                           **_summary(_rounds(ctx, variants, a.repeats, a.iters)))
    if has_out:
        dst = {f: api.Frames.empty(f, n, h, w) for f in ("nv12", "i420")}
        copy = torch.empty_like(bgr)
        variants = {"convert_" + f: (lambda f=f: api.Frames.from_bgr(ctx, bgr, None, out=dst[f]))
                    for f in dst}
        variants["device_copy_bgr"] = lambda: copy.copy_(bgr)
        conv = _summary(_rounds(ctx, variants, a.repeats, a.iters))
        px = n * w * h
        for k, v in conv.items():
            moved = 2 * 3 * px if k == "device_copy_bgr" else 3 * px + px * 3 // 2
            v["bytes_moved"] = moved
            v["gb_per_s"] = round(moved / (v["median_ms"] * 1e-3) / 1e9, 1)
        conv["measured_ceilings"] = ctx.probe_peaks()
        res["convert"] = conv
    res["bytes_written_per_frame"] = {"bgr_out": 3 * w * h, "yuv_out": w * h * 3 // 2,
                                      "bgr_out+convert": 3 * w * h + w * h * 3 // 2}
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
