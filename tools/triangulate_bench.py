"""What 3-D keypoints cost: the triangulation alone, kernel against host, and the raw-frame pipeline
with and without a rig.

    python tools/triangulate_bench.py --out profiles/triangulate/triangulate.json
    python tools/triangulate_bench.py --no-views --out profiles/triangulate/no_views_<label>.json

(1) Kernel against host.  32 time steps of a 4-camera rig with all four arrays (25 + 70 + 21 + 21
    parts): 4,384 points.  Two cases: clean detections (0.5 px noise; the leave-one-out step never
    runs) and an outlier view in every point (one view 60 px off; it always runs).  Per case and lane
    mapping -- 8 lanes per point (shipped) and a thread per point (TRI_GROUP=0), alternating --
    HIP-event milliseconds of the upload of the four keypoint arrays, of the four opk_triangulate
    calls and of the download of their results, and their sum; and opk_triangulate_host on one
    thread over the same inputs.  `--repeats` rounds; medians.
(2) The pose pipeline step (submit i + 1, collect i) on 128 frames of 1280x720, pose only and whole
    body (face and hands, 1 hand scale), seeded weights and an overlay of one synthetic person per
    frame: without views and with a 4-camera rig set, alternating in one process.  The seeded face
    and hand nets give no score above the stage's 0.35, so `whole_body` times a stage with body
    points only; `whole_body_scored` is the same with a bias on those nets' last layer, so that
    face and hand points are triangulated too (the frames are not views of one scene: the points
    are attempted, sit badly, go through the leave-one-out step and are rejected -- the expensive
    path).  `points` records, per array kind, the parts attempted per time step.

--no-views runs only the "without views" half of (2) and uses nothing this tool's commit added to
the library, so the same file measures the parent commit's library through OPK_LIB_PATH: with no
views set the rate must stay inside the spread of repeated parent runs.
"""
import argparse
import ctypes
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
from tests import cpm_graphs, prototxt                       # noqa: E402

SIZE = (1280, 720)
NET = (656, 368)
KINDS = (("body", 25), ("face", 70), ("hand_left", 21), ("hand_right", 21))
MAPPINGS = {"group": 1, "thread": 0}   # the TRI_GROUP switch: triangulate<group> (shipped), <thread>
V, STEPS = 4, 32


def _rig4():
    from tests import triangulate_cases as tc
    return tc, tc.ring_rig(np.random.default_rng(1), V, SIZE)


def kernel_against_host(ctx, repeats):
    tc, (P, sizes) = _rig4()
    tri = api.Triangulator(P, sizes)
    res = {}
    for case, noise, outlier in (("clean", 0.5, 0.0), ("outlier_in_every_point", 0.5, 60.0)):
        rng = np.random.default_rng(2)
        host_in, pinned, dev_in, dev_out, host_out = {}, {}, {}, {}, {}
        for kind, parts in KINDS:
            kp, _ = tc.scene(rng, P, STEPS, parts, noise)
            kp[:, 1, :, 0] += outlier
            host_in[kind] = kp
            pinned[kind] = torch.from_numpy(kp).pin_memory()
            dev_in[kind] = torch.empty((STEPS, V, parts, 3), device="cuda")
            dev_out[kind] = (torch.empty((STEPS, parts, 4), device="cuda"),
                            torch.empty(STEPS, dtype=torch.int32, device="cuda"))
            host_out[kind] = (torch.empty((STEPS, parts, 4)).pin_memory(),
                             torch.empty(STEPS, dtype=torch.int32).pin_memory())
        present = torch.ones((STEPS, V), dtype=torch.int32, device="cuda")
        rig = tri.struct()

        def device_round():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ctx.sync()
            ev[0].record()
            for kind, _ in KINDS:
                dev_in[kind].copy_(pinned[kind], non_blocking=True)
            ev[1].record()
            for kind, parts in KINDS:
                api.check(ctx.L.opk_triangulate(ctx.h, ctypes.byref(rig), STEPS, parts,
                                                api._ptr(dev_in[kind]), api._ptr(present),
                                                api._ptr(dev_out[kind][0]),
                                                api._ptr(dev_out[kind][1]), None, None))
            ev[2].record()
            for kind, _ in KINDS:
                host_out[kind][0].copy_(dev_out[kind][0], non_blocking=True)
                host_out[kind][1].copy_(dev_out[kind][1], non_blocking=True)
            ev[3].record()
            ctx.sync()
            up, run, down = (ev[i].elapsed_time(ev[i + 1]) for i in range(3))
            return dict(upload_ms=up, kernels_ms=run, download_ms=down, total_ms=up + run + down)

        def host_round():
            t0 = time.perf_counter()
            outs = {kind: tri.reconstruct(host_in[kind]) for kind, _ in KINDS}
            return (time.perf_counter() - t0) * 1e3, outs

        out = dict(points=STEPS * sum(p for _, p in KINDS))
        _, want = host_round()
        out["leave_one_out_points"] = int(sum((w[3] >= 0).sum() for w in want.values()))
        out["accepted_points"] = int(sum(w[0][..., 3].sum() for w in want.values()))
        rows = {m: [] for m in MAPPINGS}
        host_rows = []
        for m, switch in MAPPINGS.items():           # warm-up, and the results against the host's
            with api.dev_switches(TRI_GROUP=switch):
                device_round()
            for kind, _ in KINDS:
                assert np.array_equal(host_out[kind][0].numpy(), want[kind][0]), (case, m, kind)
                assert np.array_equal(host_out[kind][1].numpy(), want[kind][1]), (case, m, kind)
        for _ in range(repeats):
            for m, switch in MAPPINGS.items():
                with api.dev_switches(TRI_GROUP=switch):
                    rows[m].append(device_round())
            host_rows.append(host_round()[0])
        for m in MAPPINGS:
            out[m] = dict(rounds=rows[m], median={k: statistics.median(r[k] for r in rows[m])
                                                  for k in rows[m][0]})
        out["host_one_thread"] = dict(rounds_ms=host_rows, median_ms=statistics.median(host_rows))
        res[case] = out
    return res


def _net(ctx, name, graph, seed, scale, bias=0.0):
    """bias: added to the last layer of a face / hand net, so that its scores (the maxima of its
    seeded maps) pass the 3-D stage's 0.35."""
    net = api.Net(ctx, name)
    params = synth.he_weights(graph, seed=seed, out_scale=scale)
    if bias:
        w, b, slope = params["Mconv7_stage6"]
        params["Mconv7_stage6"] = (w, b + np.float32(bias), slope)
    net.set_params(params)
    return net


def _attempted(pose, tri, n):
    """Parts per time step the stage triangulated, per array kind: reconstruct() on the host over
    the collected batch's person 0, as the stage gathers them."""
    whole = api.FACE in pose._attached
    out = {}
    for kind, parts in KINDS[:4 if whole else 1]:
        kp = np.zeros((n // V, V, parts, 3), np.float32)
        present = np.zeros((n // V, V), np.int32)
        for f in range(n):
            if pose.num_people(f) < 1:
                continue
            a = {"body": lambda: pose.keypoints(f)[0], "face": lambda: pose.face_keypoints(f),
                 "hand_left": lambda: pose.hand_keypoints(f)[0],
                 "hand_right": lambda: pose.hand_keypoints(f)[1]}[kind]()
            kp[f // V, f % V], present[f // V, f % V] = a[0], 1
        _, _, errors, dropped = tri.reconstruct(kp, present)
        out[kind] = dict(attempted_per_step=float((errors >= 0).sum()) / (n // V),
                         leave_one_out_per_step=float((dropped >= 0).sum()) / (n // V))
    return out


def _cpm(name):
    return prototxt.parse(prototxt.emit(cpm_graphs.GRAPHS[name]()))


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


def pipeline(ctx, n, repeats, batches, with_views):
    res = {}
    g = torch.Generator().manual_seed(1)
    bufs = [torch.randint(0, 256, (n, SIZE[1], SIZE[0], 3), dtype=torch.uint8, generator=g).cuda()
            for _ in range(2)]
    tri = api.Triangulator(*_rig4()[1]) if with_views else None
    # whole_body_scored: the face and hand nets with a bias, so that their keypoints pass the score
    # threshold and the stage has face and hand points to triangulate (only measured with views)
    for case in ("pose", "whole_body") + (("whole_body_scored",) if tri else ()):
        nets = [_net(ctx, "builtin:BODY_25", body25.layers(), 3, 0.02)]
        pose = api.PoseExtractor(ctx, nets[0])
        pose.set_input((-1, NET[1]))
        distinct = [synth.overlay(1, NET[1] // 8, NET[0] // 8, seed=s) for s in range(8)]
        pose.set_overlay(torch.from_numpy(np.stack([distinct[f % 8] for f in range(n)])).cuda())
        exs = []
        if case != "pose":
            bias = 0.6 if case == "whole_body_scored" else 0.0
            nets += [_net(ctx, "builtin:FACE", _cpm("builtin:FACE"), 5, 0.05, bias),
                     _net(ctx, "builtin:HAND", _cpm("builtin:HAND"), 7, 0.05, bias)]
            exs = [api.KeypointExtractor(ctx, nets[1], api.FACE),
                   api.KeypointExtractor(ctx, nets[2], api.HAND)]
            for ex in exs:
                ex.set_max_batch(64)
            pose.attach(face=exs[0], hands=exs[1])
        rows = {"no_views": []}
        if tri:
            rows["views"] = []
        _step(ctx, pose, bufs, 2)
        status = points = None
        for _ in range(repeats):
            rows["no_views"].append(_step(ctx, pose, bufs, batches))
            if tri:
                pose.set_views(tri)
                rows["views"].append(_step(ctx, pose, bufs, batches))
                status = [sum(a.shape[0] for a in pose.keypoints_3d(t)) for t in range(n // V)]
                points = _attempted(pose, tri, n)
                pose.set_views(None)
        out = {k: dict(ms_per_batch=v, median_ms=statistics.median(v),
                       frames_per_s=n / statistics.median(v) * 1e3) for k, v in rows.items()}
        out["people_found_per_frame"] = statistics.mean(pose.num_people(f) for f in range(n))
        if tri:
            out["arrays_reconstructed_per_step"] = statistics.mean(status)
            out["points"] = points
        res[case] = out
        pose.close()
        for ex in exs:
            ex.close()
        for net in nets:
            net.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--no-views", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = api.Context(0)
    res = dict(frames=a.frames, size=list(SIZE), repeats=a.repeats, batches=a.batches,
               device=torch.cuda.get_device_name(0), library=os.path.basename(api._lib.LIB_PATH))
    if not a.no_views:
        res["triangulation"] = kernel_against_host(ctx, a.repeats)
    res["pipeline"] = pipeline(ctx, a.frames, a.repeats, a.batches, not a.no_views)
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
