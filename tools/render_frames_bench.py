"""Frames with skeletons on them, three ways: device time of drawing a batch of BODY_25 people on
uint8 frames and getting uint8 frames back.

    python tools/render_frames_bench.py [--frames 130] [--people 20] [--out FILE.md]

  leg A  the chain without the output-image entry points: cvmat_to_input(normalize=0) -> permute to
         contiguous HWC -> one render_pose_keypoints per frame -> round / clamp / to(uint8) in torch;
  leg B  cvmat_to_output -> one render_pose_keypoints per frame -> output_to_cvmat;
  leg C  render_frames (one geometry launch and one fused launch for the batch).

1280x720 frames at scale 1 and at scale 0.5 (to 640x360).  Per leg 10 warm-up and 50 timed
repetitions between one pair of device events on the context's stream; three repeats with the legs
alternated in one process.  Also printed: leg C's compulsory bytes (every source byte read once,
every output byte written once) over its time, next to the streaming HBM read rate that
opk_probe_peaks measures in the same run.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openpose_amd import synth                                        # noqa: E402
from openpose_amd.api import LAYER_POSE, Context, RenderLayer          # noqa: E402

W, H = 1280, 720
WARMUP, TIMED, REPEATS = 10, 50, 3


def people(n_frames, per_frame, w, h, seed):
    """[n_frames * per_frame, 25, 3] synthetic BODY_25 skeletons in w x h pixels, score 0.9."""
    kp = np.zeros((n_frames * per_frame, 25, 3), np.float32)
    for f in range(n_frames):
        kp[f * per_frame:(f + 1) * per_frame, :, :2] = synth.people(per_frame, h, w, seed + f)
    kp[..., 2] = 0.9
    return kp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=130)
    ap.add_argument("--people", type=int, default=20)
    ap.add_argument("--out", default=None, help="write the table as markdown to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    ctx = Context(0)
    n = a.frames
    frames = torch.from_numpy(
        np.random.default_rng(0).integers(0, 256, (n, H, W, 3), dtype=np.uint8)).cuda()
    rows, result = [], {"frames": n, "people_per_frame": a.people, "scales": {}}
    for scale, (ow, oh) in ((1.0, (W, H)), (0.5, (W // 2, H // 2))):
        kp = torch.from_numpy(people(n, a.people, ow, oh, seed=100)).cuda()
        per = [kp[f * a.people:(f + 1) * a.people] for f in range(n)]
        layers = [RenderLayer(LAYER_POSE, kp, [a.people] * n)]

        def leg_a():
            net_in = torch.empty((n, 3, oh, ow), device="cuda")
            ctx.cvmat_to_input(net_in, frames, scale, normalize=0)
            hwc = net_in.permute(0, 2, 3, 1).contiguous()
            for f in range(n):
                ctx.render_pose_keypoints(hwc[f], per[f])
            return torch.round(hwc).clamp(0, 255).to(torch.uint8)

        def leg_b():
            img = ctx.cvmat_to_output(frames, scale, (ow, oh))
            for f in range(n):
                ctx.render_pose_keypoints(img[f], per[f])
            return ctx.output_to_cvmat(img)

        def leg_c():
            return ctx.render_frames(frames, layers, scale, (ow, oh))

        legs = (("A", leg_a), ("B", leg_b), ("C", leg_c))
        outs = {name: fn() for name, fn in legs}
        ctx.sync()
        same = {name: bool(torch.equal(outs[name], outs["C"])) for name in ("A", "B")}
        del outs
        ms = {name: [] for name, _ in legs}
        for _ in range(REPEATS):
            for name, fn in legs:
                for _ in range(WARMUP):
                    fn()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(ctx.torch_stream)
                for _ in range(TIMED):
                    fn()
                t1.record(ctx.torch_stream)
                t1.synchronize()
                ms[name].append(t0.elapsed_time(t1) / TIMED)
        nbytes = n * 3 * (W * H + ow * oh)
        gbs = [nbytes / (t * 1e-3) / 1e9 for t in ms["C"]]
        result["scales"][str(scale)] = {"out": [ow, oh], "ms_per_batch": ms,
                                        "A_equals_C": same["A"], "B_equals_C": same["B"],
                                        "C_compulsory_bytes": nbytes, "C_gbs": gbs}
        for name, _ in legs:
            rows.append("| %.1f | %dx%d | %s | %s | %.1fx |" % (
                scale, ow, oh, name, " | ".join("%.3f" % t for t in ms[name]),
                min(ms["A"]) / max(ms[name])))
        rows.append("| %.1f | %dx%d | C GB/s | %s | |" % (
            scale, ow, oh, " | ".join("%.0f" % g for g in gbs)))
    peaks = ctx.probe_peaks()
    result["hbm_read_gbs"] = peaks["hbm_read_gbs"]
    head = ("| scale | output | leg | " + " | ".join("repeat %d (ms)" % (i + 1) for i in range(REPEATS)) +
            " | slowest vs fastest A |\n|---|---|---|" + "---|" * (REPEATS + 1))
    table = head + "\n" + "\n".join(rows)
    text = ("%d frames of %dx%d, %d BODY_25 people per frame; ms per batch, device events, %d warm-up "
            "+ %d timed repetitions per entry.\n\n%s\n\nStreaming HBM read rate probed in the same "
            "run (opk_probe_peaks): %.0f GB/s.\n" % (n, W, H, a.people, WARMUP, TIMED, table,
                                                   peaks["hbm_read_gbs"]))
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
