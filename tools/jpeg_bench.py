"""What encoding the drawn frames to JPEG costs: the encoder's passes and total against a device
copy of the same frame bytes, and the host alternatives on the same machine.

    python tools/jpeg_bench.py --out profiles/jpeg/jpeg.json

(1) The device route.  128 frames of 1280x720 BGR at quality 100 and 75, two contents: `rendered`
    (a smooth background with mild sensor noise and 20 skeletons per frame drawn by
    Context.render_frames) and `noise` (uniform random bytes, the worst case).  A round is one pair
    of HIP events around `--launches` back-to-back calls, divided by their number; `--repeats`
    rounds after a warm-up, the variants alternating, medians and the min-max spread.  The passes'
    times are differences of totals: the dev switch JPEG_PASSES stops the encoder after k launches.
    In the same rounds a device-to-device copy of the frames' bytes is the yardstick for the read.
(2) The host routes on `--host-frames` of the same frames: opk_jpeg_encode_host on 1 thread and on
    `--threads` threads (one frame per task; the call holds no Python lock), and Pillow's encoder
    (libjpeg-turbo) likewise, if Pillow imports.
"""
import argparse
import concurrent.futures as cf
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openpose_amd import api                                 # noqa: E402

SIZE = (1280, 720)
PASSES = ["jpeg_dct", "jpeg_count", "jpeg_scan_bits", "jpeg_write", "jpeg_count_ff", "jpeg_scan_ff",
          "jpeg_pack"]


def _stats(ms):
    return dict(rounds_ms=ms, median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def _timed(ctx, fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.sync()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    ctx.sync()
    return a.elapsed_time(b) / launches


def rendered_frames(ctx, n, people):
    w, h = SIZE
    rng = np.random.default_rng(4)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([96 + 64 * np.sin(x / 210.0) + y / 12.0, 110 + 50 * np.cos(y / 160.0) + x / 40.0,
                     90 + 40 * np.sin((x + y) / 300.0)], -1)
    frames = np.empty((n, h, w, 3), np.uint8)
    for f in range(n):
        frames[f] = np.clip(base + 2.0 * f / n + rng.integers(-3, 4, base.shape), 0, 255)
    centres = rng.uniform([150, 150], [w - 150, h - 150], (n * people, 1, 2))
    kp = np.concatenate([centres + rng.uniform(-140, 140, (n * people, 25, 2)),
                         np.full((n * people, 25, 1), 0.9)], -1).astype(np.float32)
    layer = api.RenderLayer(api.LAYER_POSE, torch.from_numpy(kp).cuda(), [people] * n)
    out = ctx.render_frames(torch.from_numpy(frames).cuda(), [layer])
    ctx.sync()
    return out


def device(ctx, frames, qualities, repeats, launches):
    nbytes = frames.numel()
    copy = torch.empty_like(frames)
    res = {}
    for q in qualities:
        batch = ctx.encode_jpeg(frames, q)
        sizes = batch.sizes
        calls = {"device_copy": lambda: copy.copy_(frames)}
        for k in range(1, 8):
            def call(k=k, q=q, batch=batch):
                with api.dev_switches(JPEG_PASSES=k):
                    ctx.encode_jpeg(frames, q, out=batch)
            calls["passes_%d" % k] = call
        calls["encode"] = lambda q=q, batch=batch: ctx.encode_jpeg(frames, q, out=batch)
        for c in calls.values():
            c()
        rows = {name: [] for name in calls}
        for _ in range(repeats):
            for name, c in calls.items():
                rows[name].append(_timed(ctx, c, launches))
        r = {name: _stats(ms) for name, ms in rows.items()}
        med = lambda name: r[name]["median_ms"]
        r["per_pass_ms"] = {p: med("passes_%d" % (i + 1)) - (med("passes_%d" % i) if i else 0.0)
                            for i, p in enumerate(PASSES)}
        r["output_bytes"] = int(sizes.sum())
        r["output_bytes_per_frame"] = float(sizes.mean())
        r["frame_bytes"] = nbytes
        r["read_gbs"] = nbytes / med("encode") / 1e6
        r["copy_read_gbs"] = nbytes / med("device_copy") / 1e6
        r["times_device_copy"] = med("encode") / med("device_copy")
        r["frames_per_s"] = frames.shape[0] / med("encode") * 1e3
        ctx.encode_jpeg(frames, q, out=batch)   # leave a whole batch behind, and check it
        files = batch.tobytes_list()
        assert all(f[:2] == b"\xff\xd8" and f[-2:] == b"\xff\xd9" for f in files)
        res["q%d" % q] = r
    return res


def host(frames_np, qualities, threads):
    n = frames_np.shape[0]
    hctx = api.Context.host_only()
    res = {}

    def ours(f, q):
        return len(hctx.encode_jpeg(frames_np[f:f + 1], q).bytes(0))

    routes = {"opk_jpeg_encode_host": ours}
    try:
        from PIL import Image

        def pillow(f, q):
            buf = io.BytesIO()
            Image.fromarray(frames_np[f][..., ::-1]).save(buf, "JPEG", quality=q, subsampling=2)
            return buf.tell()
        routes["pillow"] = pillow
        res["pillow"] = "present"
    except ImportError:
        res["pillow"] = "absent"
    for q in qualities:
        r = {}
        for name, fn in routes.items():
            fn(0, q)
            t = time.perf_counter()
            total = sum(fn(f, q) for f in range(n))
            one = (time.perf_counter() - t) * 1e3 / n
            with cf.ThreadPoolExecutor(threads) as ex:
                t = time.perf_counter()
                total_t = sum(ex.map(lambda f: fn(f, q), range(n)))
                many = (time.perf_counter() - t) * 1e3 / n
            assert total == total_t
            r[name] = dict(ms_per_frame_1_thread=one, ms_per_frame_threads=many, threads=threads,
                           frames_per_s_1_thread=1e3 / one, frames_per_s_threads=1e3 / many,
                           bytes_per_frame=total / n)
        res["q%d" % q] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--people", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--host-frames", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = api.Context(0)
    qualities = (100, 75)
    res = dict(frames=a.frames, size=list(SIZE), repeats=a.repeats, launches_per_round=a.launches,
               device=torch.cuda.get_device_name(0), library=os.path.basename(api._lib.LIB_PATH))
    g = torch.Generator().manual_seed(1)
    contents = {
        "rendered": rendered_frames(ctx, a.frames, a.people),
        "noise": torch.randint(0, 256, (a.frames, SIZE[1], SIZE[0], 3), dtype=torch.uint8, generator=g).cuda(),
    }
    res["device"] = {name: device(ctx, fr, qualities, a.repeats, a.launches) for name, fr in contents.items()}
    res["host"] = {name: host(fr[:a.host_frames].cpu().numpy(), qualities, a.threads)
                   for name, fr in contents.items()}
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
