"""What person ids cost: the tracker alone, and the raw-frame pipeline with and without it.

    python tools/tracking_bench.py --out profiles/tracking/tracking.json
    python tools/tracking_bench.py --pose-only --out profiles/tracking/pose_only_<label>.json

Workload: 130 frames of 1280x720, 5 and 20 people per frame, BGR and NV12.

(1) Tracker.update on the whole batch: every person is 25 keypoints that drift by up to 2 px per
    frame over smooth textured frames (so Lucas-Kanade has gradients to follow); the tracker's own
    hooks report the device milliseconds of the pyramid and of the LK launches -- for both lane
    mappings built, a wave per point (shipped) and a thread per point (LK_WAVE=0), alternating --
    and the host milliseconds of capture, bookkeeping and matching; device_bytes is what one
    tracker holds.  `--repeats` rounds, each a fresh tracker state; medians.
(2) The pose pipeline step (submit i + 1, collect i; seeded BODY_25 weights, an overlay of 5 or 20
    synthetic people) with no tracker attached and with one, alternating in one process.

--pose-only runs only the "no tracker" half of (2) and uses nothing this tool's commit added to the
library, so the same file measures the parent commit's library through OPK_LIB_PATH: the branch
collect() gained for the tracker must stay inside the spread of repeated parent runs.
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
OUT = (82, 46)   # the net output of the 656 x 368 net input
MAPPINGS = {"wave": 1, "thread": 0}   # the LK_WAVE switch: lk_points<wave> (shipped), <thread>


def _texture(seed):
    """One smooth 1280 x 720 BGR frame (bilinear noise at two scales)."""
    g = torch.Generator().manual_seed(seed)
    w, h = SIZE
    out = torch.zeros((1, 3, h, w))
    for cell, amp in ((8, 70.0), (24, 50.0)):
        coarse = torch.rand((1, 3, h // cell + 2, w // cell + 2), generator=g) * 2 - 1
        out += amp * torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear",
                                                     align_corners=False)
    return (out + 128).clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0).contiguous()


def _frames(n, seed):
    """n frames: one texture rolled by (2, 1) pixels per frame."""
    base = _texture(seed)
    return torch.stack([torch.roll(base, (f, 2 * f), (0, 1)) for f in range(n)]).cuda()


def _keypoints(n, people, seed):
    rng = np.random.default_rng(seed)
    w, h = SIZE
    centre = np.stack([rng.uniform(150, w - 150, people), rng.uniform(150, h - 150, people)], 1)
    shape = rng.uniform(-80, 80, (people, 25, 2))
    out = []
    for f in range(n):
        kp = np.zeros((people, 25, 3), np.float32)
        kp[:, :, :2] = centre[:, None] + shape + (2 * f, f) + rng.uniform(-1, 1, (people, 25, 2))
        kp[:, :, 2] = 0.9
        out.append(kp[rng.permutation(people)])
    return out


def tracker_alone(ctx, n, repeats):
    res = {}
    bgr = _frames(n, 1)
    sets = {"bgr": bgr, "nv12": api.Frames.from_bgr(ctx, bgr, "nv12")}
    for people in (5, 20):
        kps = _keypoints(n, people, people)
        for fmt, frames in sets.items():
            t = api.Tracker(ctx)
            t.set_timing(True)
            out = dict(points=n * people * 25)
            for mapping, switch in MAPPINGS.items():   # the two alternate round by round
                with api.dev_switches(LK_WAVE=switch), api.launch_log() as log:
                    t.reset()
                    t.update(frames, kps)
                t.read_times()
                kernels = [k for _, k in log]
                out[mapping] = dict(rounds=[], kernels=sorted(set(kernels)),
                                    lk_launches=kernels.count("lk_points<%s>" % mapping))
            for _ in range(repeats):
                for mapping, switch in MAPPINGS.items():
                    with api.dev_switches(LK_WAVE=switch):
                        t.reset()
                        ctx.sync()
                        t0 = time.perf_counter()
                        ids = t.update(frames, kps)
                        wall = (time.perf_counter() - t0) * 1e3
                    out[mapping]["rounds"].append(dict(t.read_times(), wall_ms=wall))
                    out[mapping]["distinct_ids"] = len({int(i) for a in ids for i in a})
            for mapping in MAPPINGS:
                rows = out[mapping]["rounds"]
                out[mapping]["median"] = {k: statistics.median(r[k] for r in rows)
                                          for k in ("pyramid_ms", "lk_ms", "host_ms", "wall_ms")}
                out["device_bytes"] = rows[-1]["device_bytes"]
            res["%s_%dpeople" % (fmt, people)] = out
            t.close()
    return res


def _rig(ctx, n, people):
    net = api.Net(ctx, "builtin:BODY_25")
    net.set_params(synth.he_weights(body25.layers(), seed=3, out_scale=0.02))
    pose = api.PoseExtractor(ctx, net)
    pose.set_input((-1, 368))
    field = synth.overlay(people, OUT[1], OUT[0], seed=people)
    pose.set_overlay(torch.from_numpy(field[None]).cuda().expand(n, -1, -1, -1).contiguous())
    return net, pose


def _step(ctx, pose, bufs, batches):
    ctx.sync()
    t0 = time.perf_counter()
    pose.submit_frames(bufs[0])
    for b in range(1, batches):
        pose.submit_frames(bufs[b & 1])
        pose.collect()
    pose.collect()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / batches


def pipeline(ctx, n, repeats, batches, with_tracker):
    res = {}
    bgr = [_frames(n, 2), _frames(n, 3)]   # two buffers: batch b - 1's frames stay until its collect
    sets = {"bgr": bgr, "nv12": [api.Frames.from_bgr(ctx, f, "nv12") for f in bgr]}
    for people in (5, 20):
        net, pose = _rig(ctx, n, people)
        tracker = api.Tracker(ctx) if with_tracker else None
        for fmt, bufs in sets.items():
            rows = {"pose_only": []}
            _step(ctx, pose, bufs, 2)
            if tracker:
                rows["tracked"], rows["tracked_thread_mapping"] = [], []
                tracker.set_timing(True)
            times = []
            for _ in range(repeats):
                rows["pose_only"].append(_step(ctx, pose, bufs, batches))
                if tracker:
                    pose.attach(tracker=tracker)
                    tracker.reset()
                    rows["tracked"].append(_step(ctx, pose, bufs, batches))
                    times.append(pose.read_track_times())
                    found = [pose.num_people(f) for f in range(n)]
                    with api.dev_switches(LK_WAVE=0):
                        tracker.reset()
                        rows["tracked_thread_mapping"].append(_step(ctx, pose, bufs, batches))
                    pose.read_track_times()
                    pose.detach_tracker()
            out = {k: dict(ms_per_batch=v, median_ms=statistics.median(v),
                           frames_per_s=n / statistics.median(v) * 1e3) for k, v in rows.items()}
            if tracker:
                out["track_times_per_batch"] = {
                    k: statistics.median(t[k] / max(t["batches"], 1) for t in times)
                    for k in ("pyramid_ms", "lk_ms", "host_ms")}
                out["people_found_per_frame"] = statistics.mean(found)
                out["device_bytes"] = tracker.read_times()["device_bytes"]
            res["%s_%dpeople" % (fmt, people)] = out
        if tracker:
            tracker.close()
        pose.close()
        net.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=130)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--pose-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = api.Context(0)
    res = dict(frames=a.frames, size=list(SIZE), repeats=a.repeats, batches=a.batches,
               device=torch.cuda.get_device_name(0), library=os.path.basename(api._lib.LIB_PATH))
    if not a.pose_only:
        res["tracker"] = tracker_alone(ctx, a.frames, a.repeats)
    res["pipeline"] = pipeline(ctx, a.frames, a.repeats, a.batches, not a.pose_only)
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
