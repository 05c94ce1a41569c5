"""What undistorting the rig's frames costs: the remap kernel alone against a device copy, and the
raw-frame pipeline with and without the stage.

    python tools/undistort_bench.py --out profiles/undistort/undistort.json
    python tools/undistort_bench.py --no-cameras --out profiles/undistort/no_cameras_<label>.json

(1) The kernel.  128 frames of 1280x720 from a 4-camera rig (the example lens's 8 coefficients, a
    5-coefficient barrel, a 12-coefficient lens, a pincushion; 128, not the 130 of bench.py: a batch
    holds whole time steps), BGR and NV12 sources.  Per source format both lane mappings (UNDISTORT_VEC:
    4 pixels per lane, or one), alternating in one process, HIP-event milliseconds per call; in the
    same rounds a device-to-device copy of the BGR frame bytes (the floor: 3 bytes read and 3 written
    per pixel, no maps, no gather) and, for NV12, opk_frames_to_bgr.  `--repeats` rounds, medians and
    the min-max spread.  gbs_algorithmic = (3 + 3 + 6) bytes per pixel over the median.
(2) The pose pipeline step (submit i + 1, collect i) on the same frames, pose only: without cameras,
    with them, with a 4-view rig set (set_views) and with both, alternating.

--no-cameras runs only the "without cameras" rows of (2) and uses nothing this tool's commit added
to the library, so the same file measures the parent commit's library through OPK_LIB_PATH.
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
NET = (656, 368)
V = 4
MAPPINGS = {"vec": 1, "plain": 0}   # the UNDISTORT_VEC switch (unset: vec for BGR, plain for YUV)


def _cameras():
    from tests import undistort_cases as uc
    K = uc.small_k(*SIZE)
    return api.Cameras([K] * V, [uc.D8_EXAMPLE, uc.D5_BARREL, uc.D12, uc.D4_PINCUSHION], [SIZE] * V)


def _summary(ms, pixels=None):
    med = statistics.median(ms)
    out = dict(rounds_ms=ms, median_ms=med, min_ms=min(ms), max_ms=max(ms))
    if pixels:
        out["gbs_algorithmic"] = pixels * 12 / med / 1e6
    return out


def _timed(ctx, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.sync()
    a.record()
    fn()
    b.record()
    ctx.sync()
    return a.elapsed_time(b)


def kernel(ctx, n, repeats):
    cams = _cameras()
    g = torch.Generator().manual_seed(1)
    bgr = torch.randint(0, 256, (n, SIZE[1], SIZE[0], 3), dtype=torch.uint8, generator=g).cuda()
    nv12 = api.Frames.from_bgr(ctx, bgr, "nv12")
    out = torch.empty_like(bgr)
    copy_dst = torch.empty_like(bgr)
    pixels = n * SIZE[0] * SIZE[1]
    res = dict(frames=n, views=V, pixels=pixels)
    for fmt, src in (("bgr", bgr), ("nv12", nv12)):
        calls = {}
        for m, switch in MAPPINGS.items():
            def call(switch=switch):
                with api.dev_switches(UNDISTORT_VEC=switch):
                    ctx.undistort_frames(src, cams, out=out)
            calls[m] = call
        calls["device_copy"] = lambda: copy_dst.copy_(bgr)
        if fmt == "nv12":
            calls["frames_to_bgr"] = lambda: nv12.to_bgr(ctx, out=copy_dst)
        kept = {}
        for name, call in calls.items():             # warm-up (the maps are built and uploaded here)
            call()
            if name in MAPPINGS:
                ctx.sync()
                kept[name] = out.clone()
        assert torch.equal(kept["vec"], kept["plain"]), fmt
        rows = {name: [] for name in calls}
        for _ in range(repeats):
            for name, call in calls.items():
                rows[name].append(_timed(ctx, call))
        r = {name: _summary(ms, pixels if name in MAPPINGS else None) for name, ms in rows.items()}
        for m in MAPPINGS:
            r[m]["times_device_copy"] = r[m]["median_ms"] / r["device_copy"]["median_ms"]
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


def pipeline(ctx, n, repeats, batches, with_cameras):
    g = torch.Generator().manual_seed(1)
    bufs = [torch.randint(0, 256, (n, SIZE[1], SIZE[0], 3), dtype=torch.uint8, generator=g).cuda()
            for _ in range(2)]
    net = api.Net(ctx, "builtin:BODY_25")
    net.set_params(synth.he_weights(body25.layers(), seed=3, out_scale=0.02))
    pose = api.PoseExtractor(ctx, net)
    pose.set_input((-1, NET[1]))
    distinct = [synth.overlay(1, NET[1] // 8, NET[0] // 8, seed=s) for s in range(8)]
    pose.set_overlay(torch.from_numpy(np.stack([distinct[f % 8] for f in range(n)])).cuda())
    settings = {"plain": (False, False)}
    if with_cameras:
        from tests import triangulate_cases as tc
        cams = _cameras()
        tri = api.Triangulator(*tc.ring_rig(np.random.default_rng(1), V, SIZE))
        settings.update({"undistort": (True, False), "views": (False, True),
                         "undistort_and_views": (True, True)})
    rows = {k: [] for k in settings}
    _step(ctx, pose, bufs, 2)
    for r in range(repeats + 1):                     # round 0 warms every setting up
        for name, (und, views) in settings.items():
            if with_cameras:
                pose.set_undistort(cams if und else None)
                pose.set_views(tri if views else None)
            ms = _step(ctx, pose, bufs, batches)
            if r:
                rows[name].append(ms)
    out = {k: dict(ms_per_batch=v, median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v),
                   frames_per_s=n / statistics.median(v) * 1e3) for k, v in rows.items()}
    out["people_found_per_frame"] = statistics.mean(pose.num_people(f) for f in range(n))
    pose.close()
    net.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--no-cameras", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.frames % V == 0, "whole time steps of the %d-camera rig" % V
    ctx = api.Context(0)
    res = dict(frames=a.frames, size=list(SIZE), repeats=a.repeats, batches=a.batches,
               device=torch.cuda.get_device_name(0), library=os.path.basename(api._lib.LIB_PATH))
    if not a.no_cameras:
        res["kernel"] = kernel(ctx, a.frames, a.repeats)
    res["pipeline"] = pipeline(ctx, a.frames, a.repeats, a.batches, not a.no_cameras)
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
