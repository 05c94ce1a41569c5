"""GPU: opk_jpeg_encode (kernels/jpeg.hip) as files, byte for byte: against the numpy restatement
(tests/jpeg_cases.py, itself held to libjpeg-turbo) at the edge sizes, on noise, flat, gradient and
ZRL frames at qualities 100 and 75, one frame and three different frames (the packed offsets), with
tight and padded steps and a base pointer off by 1 and 2 bytes (the byte path of jpeg_dct); NV12 and
I420 sources against the file of Frames.to_bgr; past the restatement's reach against the host route
at sizes that cross the kernels' scan and segment boundaries; a capacity that cuts the batch; two
runs; and PoseExtractor.write_images.  Nothing here reads outside the tree."""
import ctypes

import numpy as np
import pytest
import torch

from openpose_amd import api, synth
from openpose_amd.api import Frames, PoseExtractor
from tests import jpeg_cases as jc

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (8, 8), (16, 16), (17, 23), (24, 8), (8, 40), (7, 64), (50, 33), (90, 160)]
CONTENT = {
    "noise": lambda w, h, k: jc.noise(w, h, 100 + k),
    "flat0": lambda w, h, k: jc.flat(w, h, 0),
    "flat255": lambda w, h, k: jc.flat(w, h, 255),
    "gradient": lambda w, h, k: np.roll(jc.gradient(w, h), k, axis=2),
    "zrl": lambda w, h, k: jc.zrl_image(w, h),
}
_WANT = {}


def want(im, q):
    """The restatement's file, computed once per (frame, quality)."""
    key = (im.shape, im.tobytes(), q)
    if key not in _WANT:
        _WANT[key] = jc.encode(im, q)
    return _WANT[key]


def host_files(frames, q):
    return api.Context.host_only().encode_jpeg(frames, q).tobytes_list()


def device_frames(frames, pad=0, offset=0):
    """frames [n, h, w, 3] on the device as a BGR Frames: rows padded by `pad` bytes, the first
    byte `offset` bytes into the allocation."""
    n, h, w, _ = frames.shape
    step = w * 3 + pad
    host = np.full(offset + n * h * step, 0xA5, np.uint8)
    host[offset:].reshape(n, h, step)[:, :, :w * 3] = frames.reshape(n, h, w * 3)
    flat = torch.from_numpy(host).cuda()
    return Frames.bgr(flat[offset:].view(n, h, step), w), flat


@pytest.mark.parametrize("quality", [100, 75])
@pytest.mark.parametrize("content", sorted(CONTENT))
def test_files_equal_the_restatement(ctx, content, quality):
    """Every size, n = 1 and n = 3 with different content per frame."""
    for w, h in SIZES:
        frames = np.stack([CONTENT[content](w, h, k) for k in range(3)])
        if content == "noise":
            frames[1] = jc.gradient(w, h)   # files of different lengths inside one batch
        expect = [want(f, quality) for f in frames]
        one = ctx.encode_jpeg(torch.from_numpy(frames[:1]).cuda(), quality)
        assert one.tobytes_list() == expect[:1], (w, h)
        three = ctx.encode_jpeg(torch.from_numpy(frames).cuda(), quality)
        assert three.tobytes_list() == expect, (w, h)
        assert three.offsets[0] == 0 and three.sizes.tolist() == [len(e) for e in expect]
        assert three.bytes(2) == expect[2]


@pytest.mark.parametrize("pad,offset", [(0, 0), (4, 0), (1, 0), (0, 1), (0, 2), (5, 3), (4, 4)])
def test_steps_and_base_alignment(ctx, pad, offset):
    """Dword rows need every frame base and row step on 4 bytes (w * 3 + pad, h * step, offset):
    everything else takes the byte path; the files are the same."""
    for w, h in [(17, 23), (48, 20), (90, 160)]:
        frames = np.stack([jc.noise(w, h, 7), jc.gradient(w, h)])
        src, _keep = device_frames(frames, pad, offset)
        step = w * 3 + pad
        dwords = offset % 4 == 0 and step % 4 == 0 and (h * step) % 4 == 0
        with api.launch_log() as log:
            got = ctx.encode_jpeg(src, 75)
        names = [k for _, k in log]
        assert names[0] == ("jpeg_dct<dwords>" if dwords else "jpeg_dct<bytes>"), names
        assert names[1:] == ["jpeg_count", "jpeg_scan_bits", "jpeg_write", "jpeg_count_ff",
                             "jpeg_scan_ff", "jpeg_pack"]
        assert got.tobytes_list() == [want(f, 75) for f in frames], (w, h)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_yuv_sources_give_the_file_of_to_bgr(ctx, fmt):
    w, h = 34, 18
    bgr = torch.from_numpy(np.stack([jc.noise(w, h, 21), jc.gradient(w, h)])).cuda()
    src = Frames.from_bgr(ctx, bgr, fmt)
    back = src.to_bgr(ctx)
    got = ctx.encode_jpeg(src, 100)
    ctx.sync()
    assert got.tobytes_list() == [want(f, 100) for f in back.cpu().numpy()]


def test_against_the_host_route_across_the_kernels_boundaries(ctx):
    """Launch constants: jpeg_dct 4 MCUs per workgroup, kJpegSegMcus 8 MCUs per segment, scans in
    tiles of 256 segments / pieces, kJpegPackBytes 4096.
    656 x 368 x 2 noise: 943 MCUs = 235 * 4 + 3 (a jpeg_dct wave past the end) = 117 * 8 + 7 (a short
    last segment); about 115 pieces per frame; frame 1 starts at an odd packed offset.
    1280 x 720 rendered-like, noise on top: 3600 MCUs = 450 segments (two tiles of jpeg_scan_bits)
    and more than 256 pieces (two tiles of jpeg_scan_ff) -- asserted below."""
    small = np.stack([jc.noise(656, 368, 31), jc.noise(656, 368, 32)])
    got = ctx.encode_jpeg(torch.from_numpy(small).cuda(), 100)
    assert got.tobytes_list() == host_files(small, 100)
    y, x = np.mgrid[0:720, 0:1280]
    base = np.stack([(x // 5) % 256, (y // 3) % 256, ((x + y) // 8) % 256], -1)
    base[(np.abs(x - 2 * y) < 6) | (np.abs(x + y - 900) < 6)] = (0, 255, 85)   # drawn limbs
    big = np.clip(base + np.random.default_rng(33).integers(-90, 91, base.shape), 0, 255)
    big = big.astype(np.uint8)[None]
    got = ctx.encode_jpeg(torch.from_numpy(big).cuda(), 100)
    files = got.tobytes_list()
    assert files == host_files(big, 100)
    stuffed = files[0].count(b"\xff\x00")
    assert (len(files[0]) - 625 - stuffed) / 4096 > 256
    got75 = ctx.encode_jpeg(torch.from_numpy(big).cuda(), 75)
    assert got75.tobytes_list() == host_files(big, 75)


def test_a_capacity_that_cuts_the_batch(ctx):
    frames = np.stack([jc.noise(50, 33, k) for k in range(3)])
    expect = [want(f, 100) for f in frames]
    ends = np.cumsum([len(e) for e in expect])
    cap = int(ends[0]) + (int(ends[1]) - int(ends[0])) // 2   # between frame 0's and frame 1's end
    guard = 4096
    data = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(4, dtype=torch.int64, device="cuda")
    s = Frames.bgr(torch.from_numpy(frames).cuda()).struct()
    rc = ctx.L.opk_jpeg_encode(ctx.h, ctypes.c_void_p(data.data_ptr()), cap,
                               ctypes.c_void_p(offsets.data_ptr()), ctypes.byref(s), 100)
    assert rc == 0
    ctx.sync()
    assert offsets.cpu().numpy().tolist() == [0] + ends.tolist()   # the true ones
    host = data.cpu().numpy()
    assert host[:ends[0]].tobytes() == expect[0]
    assert (host[ends[0]:] == 0xA5).all()   # nothing from offsets[1] on, nor past the capacity
    with pytest.raises(api.OpkError, match="need %d bytes" % ends[2]):
        ctx.encode_jpeg(torch.from_numpy(frames).cuda(), 100, capacity=cap)
    # capacity 0: nothing at all
    data.fill_(0xA5)
    rc = ctx.L.opk_jpeg_encode(ctx.h, ctypes.c_void_p(data.data_ptr()), 0,
                               ctypes.c_void_p(offsets.data_ptr()), ctypes.byref(s), 100)
    ctx.sync()
    assert rc == 0 and (data.cpu().numpy() == 0xA5).all()
    assert offsets.cpu().numpy().tolist() == [0] + ends.tolist()


def test_errors_launch_nothing(ctx):
    frames = torch.from_numpy(jc.noise(16, 16, 1)[None]).cuda()
    data = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    offsets = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    s = Frames.bgr(frames).struct()
    dp, op = ctypes.c_void_p(data.data_ptr()), ctypes.c_void_p(offsets.data_ptr())
    L = ctx.L
    with api.launch_log() as log:
        assert L.opk_jpeg_encode(ctx.h, dp, 4096, op, ctypes.byref(s), 0) == 1
        assert L.opk_jpeg_encode(ctx.h, dp, 4096, op, ctypes.byref(s), 101) == 1
        assert L.opk_jpeg_encode(ctx.h, None, 4096, op, ctypes.byref(s), 100) == 1
        assert L.opk_jpeg_encode(ctx.h, dp, 4096, None, ctypes.byref(s), 100) == 1
        assert L.opk_jpeg_encode(ctx.h, ctypes.c_void_p(frames.data_ptr()), 4096, op,
                                 ctypes.byref(s), 100) == 1   # dst overlaps the source
        bad = Frames.bgr(frames).struct()
        bad.step[0] = 5
        assert L.opk_jpeg_encode(ctx.h, dp, 4096, op, ctypes.byref(bad), 100) == 1
        bad = Frames.bgr(frames).struct()
        bad.width = 65536
        bad.step[0] = 65536 * 3
        assert L.opk_jpeg_encode(ctx.h, dp, 4096, op, ctypes.byref(bad), 100) == 1
        bad = Frames.bgr(frames).struct()
        bad.height = 0
        assert L.opk_jpeg_encode(ctx.h, dp, 4096, op, ctypes.byref(bad), 100) == 1
        bad = Frames.bgr(frames).struct()
        bad.format = 7
        assert L.opk_jpeg_encode(ctx.h, dp, 4096, op, ctypes.byref(bad), 100) == 1
        none = Frames.bgr(frames).struct()
        none.n = 0
        assert L.opk_jpeg_encode(ctx.h, None, 0, None, ctypes.byref(none), 100) == 0   # n == 0
    ctx.sync()
    assert log == []
    assert (data.cpu().numpy() == 0xA5).all() and (offsets.cpu().numpy() == -1).all()


def test_two_runs_give_identical_bytes(ctx):
    frames = torch.from_numpy(np.stack([jc.noise(200, 120, k) for k in range(20)])).cuda()
    a = ctx.encode_jpeg(frames, 100)   # 20 frames: two chunks of the encoder
    b = ctx.encode_jpeg(frames, 100)
    ctx.sync()
    assert a.data.data_ptr() != b.data.data_ptr()
    la, lb = a.tobytes_list(), b.tobytes_list()
    assert la == lb
    assert la[:2] + la[15:17] == host_files(frames.cpu().numpy()[[0, 1, 15, 16]], 100)
    # out= reuses the buffers
    c = ctx.encode_jpeg(frames, 100, out=a)
    assert c.data.data_ptr() == a.data.data_ptr() and c.tobytes_list() == lb


def test_pose_write_images(ctx, tmp_path):
    fields = np.stack([synth.overlay(k + 2, 8, 12, seed=600 + k) for k in range(2)]).astype(np.float32)
    pose = PoseExtractor(ctx, None)
    pose.forward_net_output(torch.from_numpy(fields).cuda(), (96, 64), (96, 64))
    frames = torch.from_numpy(np.stack([jc.gradient(96, 64), jc.noise(96, 64, 5)])).cuda()
    paths = pose.write_images(str(tmp_path), ["a", "b"], frames, quality=90, alpha=0.5)
    assert [p[len(str(tmp_path)) + 1:] for p in paths] == ["a_rendered.jpg", "b_rendered.jpg"]
    drawn = pose.render_frames(frames, alpha=0.5)
    expect = ctx.encode_jpeg(drawn, 90).tobytes_list()
    assert [open(p, "rb").read() for p in paths] == expect
    assert expect == [want(f, 90) for f in drawn.cpu().numpy()]
    assert not torch.equal(drawn, frames)
    pose.close()
