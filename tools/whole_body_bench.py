"""Whole-body throughput (pose + face + hands through PoseExtractor.attach) and the lazy heat-map
copy against the materialised chain, on synthetic people.

    python tools/whole_body_bench.py --out profiles/whole_body/whole_body.json
    python tools/whole_body_bench.py --heat-copy --out profiles/whole_body/heat_copy.json
    python tools/whole_body_bench.py --trace --out profiles/whole_body/face64_trace.json

--trace starts a fresh child under `rocprofv3 --kernel-trace --stats` (the program after `--`, a
run of its own) that forwards a 64-crop face batch, and reports the time per kernel class (7x7,
3x3, 1x1 convs, pools, warp, argmax) of the last batch from the kernel trace and the launch log.

Whole body: BODY_25 at 656x368 on 1280x720 frames; people from a synth overlay (P per frame);
seeded weights (no checkpoints offline: the FLOPs and the launch plans are the real nets', the
detections are the overlay's).  Per configuration: frames/s and crops/s of a pipelined loop
(submit i + 1, collect i), read_part_times of both stages, and the face / hand nets' device time
per crop (Net.set_timing).  Heat copy: a 130-frame batch, heatmaps_copy_range against
heatmaps() + heatmaps_copy's device chain (opk_pose_heatmaps + opk_pose_heatmaps_copy), alternating,
three repeats each; every figure is a wall time around calls that end in a stream synchronisation.
"""
import argparse
import ctypes
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import body25                                    # noqa: E402
from openpose_amd import api, synth                          # noqa: E402
from tests import cpm_graphs, prototxt                       # noqa: E402

SIZE = (1280, 720)
NET = (656, 368)


def _net(ctx, name, graph, seed, scale, split):
    net = api.Net(ctx, name)
    net.set_params(synth.he_weights(graph, seed=seed, out_scale=scale))
    if split:
        net.set_precision(api.PRECISION_SPLIT)
    return net


def _cpm(name):
    return prototxt.parse(prototxt.emit(cpm_graphs.GRAPHS[name]()))


def _overlay(people, frames):
    distinct = [synth.overlay(people, NET[1] // 8, NET[0] // 8, seed=s) for s in range(min(frames, 8))]
    return torch.from_numpy(np.stack([distinct[f % len(distinct)] for f in range(frames)])).cuda()


def whole_body(ctx, frames_n, people, max_batch, split, case, batches, warmup):
    """case: pose | face | hands1 | hands6."""
    pose_net = _net(ctx, "builtin:BODY_25", body25.layers(), 3, 0.02, split)
    pose = api.PoseExtractor(ctx, pose_net)
    pose.set_input((-1, NET[1]))
    overlay = _overlay(people, frames_n)
    pose.set_overlay(overlay)
    nets, exs = {}, {}
    if case != "pose":
        nets[api.FACE] = _net(ctx, "builtin:FACE", _cpm("builtin:FACE"), 5, 0.05, split)
        exs[api.FACE] = api.KeypointExtractor(ctx, nets[api.FACE], api.FACE)
    if case.startswith("hands"):
        nets[api.HAND] = _net(ctx, "builtin:HAND", _cpm("builtin:HAND"), 7, 0.05, split)
        exs[api.HAND] = api.KeypointExtractor(ctx, nets[api.HAND], api.HAND)
        exs[api.HAND].set_scales(int(case[5:]), 0.4)
    for k, ex in exs.items():
        ex.set_max_batch(max_batch)
        nets[k].set_timing(True)
    pose.attach(face=exs.get(api.FACE), hands=exs.get(api.HAND))
    g = torch.Generator().manual_seed(1)
    bufs = [torch.randint(0, 256, (frames_n, SIZE[1], SIZE[0], 3), dtype=torch.uint8,
                          generator=g).cuda() for _ in range(2)]

    def loop(count):
        pose.submit_frames(bufs[0])
        for b in range(1, count):
            pose.submit_frames(bufs[b & 1])   # batch b - 1's frames stay until its collect
            pose.collect()
        pose.collect()

    loop(warmup)
    for k in exs:
        pose.read_part_times(k)
        nets[k].read_timing()
    pose.read_collect_times()
    ctx.sync()
    t0 = time.perf_counter()
    loop(batches)
    ctx.sync()
    dt = time.perf_counter() - t0
    res = dict(frames=frames_n, people=people, max_batch=max_batch,
               precision="split" if split else "fp16", case=case, batches=batches,
               seconds=dt, frames_per_s=frames_n * batches / dt,
               people_found=sum(pose.num_people(f) for f in range(frames_n)),
               collect=pose.read_collect_times())
    crops = 0
    for k, name in ((api.FACE, "face"), (api.HAND, "hand")):
        if k not in exs:
            continue
        t = pose.read_part_times(k)
        fw, ms = nets[k].read_timing()
        res[name] = dict(t, net_forwards=fw, net_ms=ms,
                         net_ms_per_crop=ms / t["crops"] if t["crops"] else None)
        crops += t["crops"]
    res["crops_per_s"] = crops / dt
    pose.close()
    for ex in exs.values():
        ex.close()
    for n in list(nets.values()) + [pose_net]:
        n.close()
    return res


def heat_copy(ctx, frames_n, repeats):
    """The new call against the materialised chain on one injected 130-frame batch."""
    rng = np.random.default_rng(0)
    one = (rng.standard_normal((8, 78, NET[1] // 8, NET[0] // 8)) * 0.3).astype(np.float32)
    field = torch.from_numpy(one).cuda().repeat((frames_n + 7) // 8, 1, 1, 1)[:frames_n].contiguous()
    pose = api.PoseExtractor(ctx, None)
    L = pose.L
    shape = (ctypes.c_int * 4)()
    out = []
    for label, types, mode, dtype in (("all NoScale float", 7, 8, torch.float32),
                                      ("parts UnsignedChar uint8", 1, 7, torch.uint8)):
        nsel = 78 if types == 7 else 25
        dst = torch.empty((frames_n, nsel, NET[1], NET[0]), dtype=dtype, device="cuda")
        dstf = dst if dtype == torch.float32 else torch.empty(dst.shape, dtype=torch.float32,
                                                              device="cuda")
        lazy, chain = [], []
        for r in range(repeats + 1):   # repeat 0 warms both paths up (allocations, tables)
            # a fresh collect: the chain materialises its stack once per collected batch
            pose.forward_net_output(field, NET, NET)
            ctx.sync()

            def run_lazy():
                t = time.perf_counter()
                pose.heatmaps_copy_range(types, mode, dtype=dtype, out=dst)
                return (time.perf_counter() - t) * 1e3

            def run_chain():   # (its destination is float in either case: the chain has no uint8)
                t = time.perf_counter()
                api.check(L.opk_pose_heatmaps_copy(pose.h, types, mode, api._ptr(dstf), shape))
                return (time.perf_counter() - t) * 1e3

            if r % 2:   # the order alternates from repeat to repeat
                a, b = run_lazy(), run_chain()
            else:
                b, a = run_chain(), run_lazy()
            if r:
                lazy.append(a)
                chain.append(b)
        out.append(dict(case=label, frames=frames_n, dst_bytes=dst.numel() * dst.element_size(),
                        chain_dst_bytes=dstf.numel() * 4, order="lazy first in odd repeats (1, 3), chain first in even",
                        lazy_ms=lazy, chain_ms=chain,
                        lazy_write_gbs=[dst.numel() * dst.element_size() / (m * 1e-3) / 1e9 for m in lazy]))
    pose.close()
    return out


def trace_run(launches, crops=64, split=False):
    """The traced program: a 64-crop face batch (one net forward of 64 crops at 368x368), six
    times; writes the launch log (layer, kernel) of one net forward and the convs' kernel sizes."""
    ctx = api.Context(0)
    net = _net(ctx, "builtin:FACE", _cpm("builtin:FACE"), 5, 0.05, split)
    ex = api.KeypointExtractor(ctx, net, api.FACE)
    ex.set_max_batch(crops)
    g = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 256, (1, SIZE[1], SIZE[0], 3), dtype=torch.uint8, generator=g).cuda()
    rng = np.random.default_rng(3)
    rects = np.zeros((crops, 4), np.float32)
    rects[:, 2] = rects[:, 3] = rng.uniform(60, 300, crops)
    rects[:, 0] = rng.uniform(0, SIZE[0] - 300, crops)
    rects[:, 1] = rng.uniform(0, SIZE[1] - 300, crops)
    with api.dev_switches(LAUNCH_LOG=1):
        ex.forward(frames, rects)
        log = net.launch_log()
    for _ in range(5):
        ex.forward(frames, rects)
    ctx.sync()
    with open(launches, "w") as f:
        json.dump({"log": log, "crops": crops, "precision": "split" if split else "fp16",
                   "kernel_size": {c["name"]: c["kernel_size"] for c in net.convs()}}, f)
    ex.close()
    net.close()
    ctx.close()


def trace_summary(trace_csv, launches):
    """Time per kernel class of the last traced face batch: the launches between its warp
    (cvmat_to_input) and its argmax (heat_argmax) are the net forward's, in the launch log's order."""
    import csv
    meta = json.load(open(launches))
    log, sizes = meta["log"], meta["kernel_size"]
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    warps = [i for i, r in enumerate(rows) if "cvmat_to_input" in r["Kernel_Name"]]
    first = warps[-1]
    last = next(i for i in range(first, len(rows)) if "heat_argmax" in rows[i]["Kernel_Name"])
    seg = rows[first + 1:last]
    classes, kernels = {}, {}

    def add(table, key, r):
        v = table.setdefault(key, [0, 0.0])
        v[0] += 1
        v[1] += us(r)

    add(classes, "warp (cvmat_to_input)", rows[first])
    add(classes, "argmax (heat_argmax)", rows[last])
    labelled = len(seg) == len(log) and all(k.split("<")[0] in r["Kernel_Name"]
                                            for (_, k), r in zip(log, seg))
    for i, r in enumerate(seg):
        if labelled:
            layer = log[i][0]
            k = sizes.get(layer.split("+")[0])   # (a fused unit counts as its first conv)
            add(classes, "pools" if layer == "pool" else
                ("%dx%d convs" % (k, k) if k else "other: " + layer), r)
            add(kernels, log[i][1], r)
        else:   # the trace and the log disagree: kernel names only
            add(classes, "net, unlabelled: " + r["Kernel_Name"].split("(")[0].split("<")[0], r)
    span = (int(rows[last]["End_Timestamp"]) - int(rows[first]["Start_Timestamp"])) / 1e3
    busy = sum(v[1] for v in classes.values())
    return {"crops": meta["crops"], "precision": meta["precision"], "launches": len(seg) + 2,
            "labelled_by_launch_log": labelled, "span_us": round(span, 1),
            "kernels_us": round(busy, 1), "us_per_crop": round(span / meta["crops"], 2),
            "classes_us": {k: [v[0], round(v[1], 1)] for k, v in sorted(classes.items())},
            "kernels_us_by_name": {k: [v[0], round(v[1], 1)] for k, v in sorted(kernels.items())}}


def trace(out, split):
    """One kernel-trace run of its own: a fresh child process under rocprofv3 (this process never
    opens the GPU), then the classification of its kernel trace."""
    import glob
    import subprocess
    d = os.path.splitext(os.path.abspath(out))[0] + "_trace"
    os.makedirs(d, exist_ok=True)
    launches = os.path.join(d, "launches.json")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--trace-run", launches, "--out", out]
    if split:
        cmd += ["--precision", "split"]
    subprocess.run(cmd, check=True, timeout=600)
    found = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    if not found:
        sys.exit("whole_body_bench: no kernel trace under " + d)
    res = trace_summary(found[-1], launches)
    res["command"] = " ".join(["python"] + sys.argv)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--heat-copy", action="store_true")
    ap.add_argument("--trace", action="store_true",
                    help="rocprofv3 kernel trace of a 64-crop face batch, time per kernel class")
    ap.add_argument("--trace-run", default=None, help="(the traced child of --trace)")
    ap.add_argument("--frames", type=int, nargs="+", default=[130, 16])
    ap.add_argument("--people", type=int, nargs="+", default=[1, 5, 20])
    ap.add_argument("--max-batch", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--precision", nargs="+", default=["fp16", "split"])
    ap.add_argument("--cases", nargs="+", default=["pose", "face", "hands1", "hands6"])
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.trace_run:
        return trace_run(a.trace_run, split=a.precision == ["split"])
    if a.trace:
        return trace(a.out, split=a.precision == ["split"])
    ctx = api.Context(0)
    results = []
    if a.heat_copy:
        results = heat_copy(ctx, a.frames[0], a.repeats)
    else:
        for fr, p, prec, case in itertools.product(a.frames, a.people, a.precision, a.cases):
            for mb in (a.max_batch if case != "pose" else a.max_batch[:1]):
                r = whole_body(ctx, fr, p, mb, prec == "split", case, a.batches, a.warmup)
                print(json.dumps(r), flush=True)
                results.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(command=" ".join(["python"] + sys.argv), results=results), f, indent=1)
    for r in results:
        print(json.dumps(r))
    ctx.close()


if __name__ == "__main__":
    main()
