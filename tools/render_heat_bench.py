"""Frames with a heat map or PAF overlay (--part_to_show), two ways: device time and device memory
of drawing one element of a collected BODY_25 batch on uint8 frames and getting uint8 frames back.

    python tools/render_heat_bench.py [--frames 130] [--out FILE.md] [--json FILE.json]

  leg A  the chain of the per-frame entry points: materialise the full-resolution heat stack
         [n][78][368][656] (resize_and_merge of the net output, what opk_pose_heatmaps runs) ->
         cvmat_to_output (float frames) -> one render_heat_map / render_heat_maps / render_pafs per
         frame -> output_to_cvmat;
  leg C  PoseExtractor.render_frames(element=...): one fused launch, heat values evaluated from the
         net output, a tile's window staged in LDS;
  leg P  leg C with the dev switch RENDER_HEAT_STAGE=0: every pixel evaluates its own samples.

1280x720 frames, a random injected net output [n][78][46][82] (net input 656x368; values within
+-0.045, under the NMS threshold, so that the forward that collects the batch finds nobody: none of
the timed work depends on the values), elements 1
(background), 2 (all parts), 3 (all PAFs), 4 (part 0) and 29 (the first PAF).  Per leg 2 warm-up and
5 timed repetitions between one pair of device events on the context's stream; three repeats with
the legs alternated in one process.  Peak device memory: the leg's own torch allocations
(max_memory_allocated over the leg, minus what was allocated before it); the frames and the net
output are shared and not counted.  Also printed: the heat_at evaluations per 32x8 tile of leg C
(the staged windows, restated here from kernels/render.hip) against leg P's (256 pixels x the
kind's taps).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openpose_amd.api import (HEAT_PAF, HEAT_PAFS, HEAT_PART, HEAT_PARTS, Context,   # noqa: E402
                              PoseExtractor, dev_switches, render_element)

W, H = 1280, 720
NET, OUT = (656, 368), (82, 46)
WARMUP, TIMED, REPEATS = 2, 5, 3
ELEMENTS = [(1, "background"), (2, "all parts"), (3, "all PAFs"), (4, "part 0"), (29, "PAF 0")]
# kind -> (taps below / above the base pixel, channels per pass, taps per pixel and pass)
WINDOW = {HEAT_PART: (1, 2, 1, 16), HEAT_PARTS: (0, 1, 1, 1), HEAT_PAF: (0, 1, 2, 8),
          HEAT_PAFS: (0, 0, 2, 2)}


def evaluations_per_tile(kind, passes, scale, hw, hh):
    """(staged, per pixel) heat_at evaluations of the mean full 32x8 tile: heat_window's rectangle
    in float32, as the kernel computes it."""
    lo, hi, planes, taps = WINDOW[kind]
    s = np.float32(scale)

    def base(px, size):
        v = (np.float32(px) + np.float32(0.5)) / s - np.float32(0.5)
        return int(np.clip(np.floor(v), 0, size - 1))

    def extent(first, last, size):
        return min(size - 1, base(last, size) + hi) - max(0, base(first, size) - lo) + 1

    total, tiles = 0, 0
    for ty in range(0, H, 8):
        eh = extent(ty, ty + 7, hh)
        for tx in range(0, W, 32):
            total += extent(tx, tx + 31, hw) * eh * planes
            tiles += 1
    return passes * total / tiles, passes * 256 * taps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=130)
    ap.add_argument("--out", default=None, help="write the table as markdown to this file")
    ap.add_argument("--json", default=None, help="write the result as JSON to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    ctx = Context(0)
    n = a.frames
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).cuda()
    net_out = torch.from_numpy(rng.uniform(-0.045, 0.045, (n, 78) + OUT[::-1]).astype(np.float32)).cuda()
    pose = PoseExtractor(ctx, None)
    pose.forward_net_output(net_out, NET, (W, H))
    scale = pose.scale_net_to_output()
    rows, result = [], {"frames": n, "scale_net_to_output": scale, "elements": {}}
    for element, name in ELEMENTS:
        kind, channel = render_element(0, element)
        passes = {HEAT_PARTS: 25, HEAT_PAFS: 26}.get(kind, 1)

        def leg_a():
            stack = torch.empty((n, 78, NET[1], NET[0]), dtype=torch.float32, device="cuda")
            ctx.resize_and_merge(stack, [net_out])
            img = ctx.cvmat_to_output(frames)
            for f in range(n):
                if kind == HEAT_PART:
                    ctx.render_heat_map(img[f], stack[f], scale, channel)
                elif kind == HEAT_PARTS:
                    ctx.render_heat_maps(img[f], stack[f], scale)
                else:
                    ctx.render_pafs(img[f], stack[f], scale, channel if kind == HEAT_PAF else None)
            return ctx.output_to_cvmat(img)

        def leg_c():
            return pose.render_frames(frames, element=element)

        def leg_p():
            with dev_switches(RENDER_HEAT_STAGE=0):
                return pose.render_frames(frames, element=element)

        legs = (("A", leg_a), ("C", leg_c), ("P", leg_p))
        outs, mem = {}, {}
        for leg, fn in legs:
            ctx.sync()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            outs[leg] = fn()
            ctx.sync()
            mem[leg] = torch.cuda.max_memory_allocated() - before
        same = {leg: bool(torch.equal(outs[leg], outs["C"])) for leg in ("A", "P")}
        del outs
        ms = {leg: [] for leg, _ in legs}
        for _ in range(REPEATS):
            for leg, fn in legs:
                for _ in range(WARMUP):
                    fn()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(ctx.torch_stream)
                for _ in range(TIMED):
                    fn()
                t1.record(ctx.torch_stream)
                t1.synchronize()
                ms[leg].append(t0.elapsed_time(t1) / TIMED)
        staged, per_pixel = evaluations_per_tile(kind, passes, scale, NET[0], NET[1])
        result["elements"][str(element)] = {
            "name": name, "kind": kind, "channel": channel, "ms_per_batch": ms,
            "peak_bytes": mem, "A_equals_C": same["A"], "P_equals_C": same["P"],
            "heat_at_per_tile": {"C": staged, "P": per_pixel},
            "C_slowest_below_A_fastest": max(ms["C"]) < min(ms["A"])}
        for leg, _ in legs:
            rows.append("| %d %s | %s | %s | %.2f | %.1fx | %s |" % (
                element, name, leg, " | ".join("%.3f" % t for t in ms[leg]), mem[leg] / 1e9,
                min(ms["A"]) / max(ms[leg]),
                {"A": "", "C": "%.0f" % staged, "P": "%d" % per_pixel}[leg]))
    head = ("| element | leg | " + " | ".join("repeat %d (ms)" % (i + 1) for i in range(REPEATS)) +
            " | peak GB | slowest vs fastest A | heat_at per tile |\n|---|---|" +
            "---|" * (REPEATS + 3))
    table = head + "\n" + "\n".join(rows)
    text = ("%d frames of %dx%d, BODY_25 net output %dx%d, heat scale %.4f; ms per batch, device "
            "events, %d warm-up + %d timed repetitions per entry.\n\n%s\n" % (
                n, W, H, OUT[0], OUT[1], scale, WARMUP, TIMED, table))
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(json.dumps(result))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    pose.close()


if __name__ == "__main__":
    main()
