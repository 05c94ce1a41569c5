"""Cost and keypoint parity of per-layer precision schedules (Net.set_precision_schedule): BODY_25 at
the bench geometry (656 x 368 net input from 1280 x 720 frames), He-initialised weights with
full-strength heads, as the parity block of bench.py -- whose helpers this imports.

    python tools/precision_schedule_sweep.py [--frames 24] [--rounds 3] [--out sweep.json]

Schedules: uniform fp16, uniform split, fp16 trunk + split stages, split trunk + fp16 stages, and
split in the last N stages only (stages in execution order: the four PAF stages, then the two
heat-map stages), N = 1 .. 5 (N = 6 is fp16 trunk + split stages).

Per schedule:
  * CNN ms per forward (opk_net_set_timing: HIP events around each forward) at the bench batch
    and at one frame in small-batch mode: `rounds` rounds, the schedules alternated inside each
    round of one process (so that the box's drift hits them alike), each sample the mean of three
    forwards after two warm ones; the figure is the median of the rounds, the cost relative to
    uniform split of the same run;
  * on the schedules with an fp16 -> split boundary, the same with SPLIT_XHI=0 (the three-product
    kernels over a zero twin instead of the hi-only kernels);
  * over `frames` frames against the fp32 CPU path (bench.cpu_parity): share of peaks at the
    identical pixel, share of people with every keypoint within 1e-3; meets = VERDICT.md's line,
    >= 99.9 % of peaks and >= 99 % of people.

Prints one JSON document (also written to --out) and, on stderr, the table of
profiles/precision_schedule/README.md.
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

FP16, SPLIT = 0, 1


def stage_of(name):
    """(stage, branch) of a stage conv ("Mconv3_stage1_L2_0" -> "stage1_L2"), None for the trunk."""
    if not name.startswith("Mconv"):
        return None
    parts = name.split("_")
    return parts[1] + "_" + parts[2]


def schedules(convs):
    stages = list(dict.fromkeys(s for s in (stage_of(c["name"]) for c in convs) if s))
    out = {
        "uniform_fp16": [FP16] * len(convs),
        "uniform_split": [SPLIT] * len(convs),
        "fp16_trunk_split_stages": [SPLIT if stage_of(c["name"]) else FP16 for c in convs],
        "split_trunk_fp16_stages": [FP16 if stage_of(c["name"]) else SPLIT for c in convs],
    }
    for n in range(1, len(stages)):
        last = set(stages[-n:])
        out["split_last_%d_stages" % n] = [SPLIT if stage_of(c["name"]) in last else FP16 for c in convs]
    return out, stages


def has_boundary(sched):
    """An fp16 conv before a split one (uniform schedules and a split trunk have none)."""
    return FP16 in sched and SPLIT in sched and sched.index(SPLIT) > sched.index(FP16)


def apply(net, sched):
    """The schedule, through the other uniform schedule first: the shapes are re-planned (and dev
    switches re-read) even where the schedule is the one in force."""
    net.set_precision_schedule([1 - sched[0]] * len(sched))
    net.set_precision_schedule(sched)


def time_forward(net, x):
    for _ in range(2):
        net.forward(x)
    torch.cuda.synchronize()
    net.set_timing(True)
    for _ in range(3):
        net.forward(x)
    k, ms = net.read_timing()
    net.set_timing(False)
    return ms / k


def timing(net, scheds, x, rounds, small):
    from openpose_amd.api import dev_switches
    net.set_small_batch(small)
    samples = {}
    for r in range(rounds):
        for name, sched in scheds.items():
            apply(net, sched)
            samples.setdefault(name, []).append(time_forward(net, x))
            if has_boundary(sched):
                with dev_switches(SPLIT_XHI=0):
                    apply(net, sched)
                    samples.setdefault(name + "@SPLIT_XHI=0", []).append(time_forward(net, x))
        print("timing %s round %d done" % ("1 frame small-batch" if small else "%d frames" % x.shape[0], r),
              file=sys.stderr, flush=True)
    net.set_small_batch(False)
    return {k: {"ms": round(statistics.median(v), 4), "rounds": [round(s, 4) for s in v]}
            for k, v in samples.items()}


def parity_run(net, pose, params, frames_u8, sched):
    """bench.gpu_parity_run with a schedule in place of the uniform precision."""
    net.set_params(params)
    net.set_precision_schedule(sched)
    pose.set_overlay(None)
    pose.forward_frames(frames_u8)
    n = frames_u8.shape[0]
    return {"params": params, "net_input": pose.net_input_numpy(), "net_output": net.output_numpy(),
            "peaks": pose.peaks_numpy(), "keypoints": [pose.keypoints(f)[0] for f in range(n)],
            "scale": pose.scale_net_to_output()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24, help="frames of the parity sample")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0, help="bench batch (0: bench.tile_aligned_batch)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from openpose_amd import synth
    from openpose_amd.api import Context, Net, PoseExtractor
    alive = threading.Event()

    def heartbeat():   # (the CPU reference of the parity sample prints nothing for minutes)
        t0 = time.time()
        while not alive.wait(60):
            print("... %d s" % (time.time() - t0), file=sys.stderr, flush=True)
    threading.Thread(target=heartbeat, daemon=True).start()

    ctx = Context(0)
    net = Net(ctx, "builtin:BODY_25")
    convs = net.convs()
    scheds, stages = schedules(convs)
    params = synth.he_weights(convs, seed=0, out_scale=1.0)
    net.set_params(params)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batch = a.batch or bench.tile_aligned_batch(cus)
    rng = np.random.default_rng(1)
    res = {"net": "BODY_25", "net_input": [bench.NET_H, bench.NET_W], "cus": cus, "batch": batch,
           "rounds": a.rounds, "stages_in_execution_order": stages,
           "schedules": {k: "".join("s" if p else "h" for p in v) for k, v in scheds.items()}}
    xb = torch.from_numpy(rng.uniform(-0.5, 0.5, (batch, 3, bench.NET_H, bench.NET_W)).astype(np.float32)).cuda()
    res["cnn_ms_bench_batch"] = timing(net, scheds, xb, a.rounds, small=False)
    del xb
    x1 = torch.from_numpy(rng.uniform(-0.5, 0.5, (1, 3, bench.NET_H, bench.NET_W)).astype(np.float32)).cuda()
    res["cnn_ms_one_frame_small_batch"] = timing(net, scheds, x1, a.rounds, small=True)

    # parity over a.frames frames of the bench geometry, the fp32 reference computed once
    bench.PARITY_FRAMES = a.frames
    pose = PoseExtractor(ctx, net)
    pose.set_input((-1, bench.NET_H))
    gen = torch.Generator(device="cuda").manual_seed(4321)
    frames = torch.randint(0, 256, (a.frames, 720, 1280, 3), generator=gen, device="cuda", dtype=torch.uint8)
    names = list(scheds)
    gs = [parity_run(net, pose, params, frames, scheds[k]) for k in names]
    print("parity: GPU runs done, fp32 reference of %d frames on the CPU" % a.frames, file=sys.stderr, flush=True)
    threads = bench.cpu_share()[0]
    par = bench.cpu_parity(gs, threads)
    res["parity_frames"] = a.frames
    res["parity"] = {}
    for k, p in zip(names, par):
        p.pop("per_frame", None)
        res["parity"][k] = p
    alive.set()

    # one row per schedule
    rows = []
    for k in names:
        b, o = res["cnn_ms_bench_batch"], res["cnn_ms_one_frame_small_batch"]
        p = res["parity"][k]
        row = {"schedule": k, "split_convs": sum(scheds[k]),
               "bench_ms": b[k]["ms"], "bench_cost_vs_split": round(b[k]["ms"] / b["uniform_split"]["ms"], 4),
               "one_frame_ms": o[k]["ms"], "one_frame_cost_vs_split": round(o[k]["ms"] / o["uniform_split"]["ms"], 4),
               "peaks_identical": p["peak_index_identical"], "people_within_1e-3": p["people_identical_1e-3_frac"],
               "net_rel_l2": p["net_rel_l2"]}
        if k + "@SPLIT_XHI=0" in b:
            row["bench_ms_xhi0"] = b[k + "@SPLIT_XHI=0"]["ms"]
            row["one_frame_ms_xhi0"] = o[k + "@SPLIT_XHI=0"]["ms"]
        row["meets"] = bool(row["peaks_identical"] >= 0.999 and row["people_within_1e-3"] >= 0.99)
        rows.append(row)
    res["rows"] = rows
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    hdr = ("schedule", "split convs", "ms / %d frames" % batch, "vs split", "SPLIT_XHI=0", "ms / 1 frame", "vs split",
           "SPLIT_XHI=0", "peaks identical", "people within 1e-3", "meets")
    print("| " + " | ".join(hdr) + " |\n|" + "---|" * len(hdr), file=sys.stderr)
    for r in rows:
        print("| %s | %d | %.2f | %.3f | %s | %.3f | %.3f | %s | %.2f %% | %.2f %% | %s |" % (
            r["schedule"], r["split_convs"], r["bench_ms"], r["bench_cost_vs_split"],
            "%.2f" % r["bench_ms_xhi0"] if "bench_ms_xhi0" in r else "",
            r["one_frame_ms"], r["one_frame_cost_vs_split"],
            "%.3f" % r["one_frame_ms_xhi0"] if "one_frame_ms_xhi0" in r else "",
            100 * r["peaks_identical"], 100 * r["people_within_1e-3"], "yes" if r["meets"] else "no"), file=sys.stderr)


if __name__ == "__main__":
    main()
