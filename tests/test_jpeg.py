"""CPU: the host route of the JPEG frames -- opk_jpeg_encode_host through Context.host_only()
against the numpy restatement (tests/jpeg_cases.py) byte for byte, opk_jpeg_bound, every refused
argument, a capacity that is too small, JpegBatch.save's file names -- and the same host code under
AddressSanitizer / UBSan in a stand-alone program (tests/jpeg_driver.cpp)."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest

from openpose_amd import _lib, api
from openpose_amd import build as opk_build
from tests import jpeg_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return [(name, im, q, jc.encode(im, q)) for name, im, q in jc.cases()]


@pytest.fixture(scope="module")
def host():
    ctx = api.Context.host_only()
    yield ctx
    ctx.close()


def test_host_route_equals_the_restatement(host, cases):
    for name, im, q, want in cases:
        batch = host.encode_jpeg(im[None], q)
        assert batch.bytes(0) == want, name
        assert batch.offsets.tolist() == [0, len(want)] and batch.sizes.tolist() == [len(want)]
        assert api.jpeg_bound(1, im.shape[1], im.shape[0]) >= len(want)
    for w, h in jc.SIZES:   # the Pillow sizes too, where the cases above do not have them
        im = jc.noise(w, h, 50 + w)
        assert host.encode_jpeg(im[None], 100).bytes(0) == jc.encode(im, 100), (w, h)


def test_batches_with_padded_steps_and_strides(host):
    rng = np.random.default_rng(5)
    for (w, h), q in (((17, 23), 100), ((50, 33), 75), ((8, 40), 100)):
        n, step, gap = 3, w * 3 + 7, 11
        flat = rng.integers(0, 256, n * (h * step + gap), dtype=np.uint8)
        view = np.lib.stride_tricks.as_strided(flat, (n, h, w, 3), (h * step + gap, step, 3, 1))
        before = flat.copy()
        batch = host.encode_jpeg(view, q)
        want = [jc.encode(np.ascontiguousarray(view[f]), q) for f in range(n)]
        assert batch.tobytes_list() == want
        assert batch.offsets.tolist() == [0] + np.cumsum([len(x) for x in want]).tolist()
        assert np.array_equal(flat, before)


def test_bound_holds_for_a_frame_built_for_long_codes(host, cases):
    im = jc.max_code_frame(64, 64)
    size = len(host.encode_jpeg(im[None], 100).bytes(0))
    assert size == len(jc.encode(im, 100))
    assert api.jpeg_bound(1, 64, 64) >= size
    # 16 MCUs of 6 blocks of at most 1660 bits, doubled by stuffing, plus header and EOI
    assert api.jpeg_bound(1, 64, 64) == 623 + 2 + 2 * ((96 * 1660 + 7) // 8)
    assert api.jpeg_bound(5, 64, 64) == 5 * api.jpeg_bound(1, 64, 64)
    assert api.jpeg_bound(1, 1, 1) == api.jpeg_bound(1, 16, 16) < api.jpeg_bound(1, 17, 16)
    assert api.jpeg_bound(0, 64, 64) == 0


def _encode(dst, cap, off, src, step, frame, n, w, h, q):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    return _lib.load().opk_jpeg_encode_host(p(dst), cap, p(off), p(src), step, frame, n, w, h, q)


def test_every_refused_argument_writes_nothing():
    src = jc.noise(16, 16, 1)
    dst = np.full(api.jpeg_bound(1, 16, 16), 0xA5, np.uint8)
    off = np.full(2, 77, np.uint64)
    cap = dst.size
    bad = [
        (dst, cap, off, src, 0, 0, 1, 16, 16, 0), (dst, cap, off, src, 0, 0, 1, 16, 16, 101),
        (dst, cap, off, src, 0, 0, 1, 0, 16, 100), (dst, cap, off, src, 0, 0, 1, 16, 0, 100),
        (dst, cap, off, src, 0, 0, 1, 65536, 16, 100), (dst, cap, off, src, 0, 0, 1, 16, 65536, 100),
        (dst, cap, off, src, 0, 0, -1, 16, 16, 100), (dst, cap, off, src, 47, 0, 1, 16, 16, 100),
        (dst, cap, off, src, 0, 100, 2, 16, 16, 100),
        (None, cap, off, src, 0, 0, 1, 16, 16, 100), (dst, cap, None, src, 0, 0, 1, 16, 16, 100),
        (dst, cap, off, None, 0, 0, 1, 16, 16, 100),
        (src, src.size, off, src, 0, 0, 1, 16, 16, 100),          # dst is the source
        (src[4:], 8, off, src, 0, 0, 1, 16, 16, 100),             # dst inside the source
    ]
    for args in bad:
        assert _encode(*args) == 1, args[4:]
        assert _lib.load().opk_last_error()
    assert (dst == 0xA5).all() and off.tolist() == [77, 77]
    assert np.array_equal(src, jc.noise(16, 16, 1))
    assert _encode(None, 0, off, None, 0, 0, 0, 16, 16, 100) == 0 and off[0] == 0   # n == 0
    with pytest.raises(api.OpkError, match="quality"):
        api.Context.host_only().encode_jpeg(src[None], 0)


def test_a_capacity_that_is_too_small_gives_true_offsets(host):
    frames = np.stack([jc.noise(50, 33, k) for k in range(3)])
    want = [jc.encode(f, 100) for f in frames]
    ends = np.cumsum([len(x) for x in want]).tolist()
    guard = 64
    for cap in (0, 1, ends[0] - 1, ends[0], ends[0] + 1, ends[1] - 1, ends[1], ends[2] - 1, ends[2]):
        dst = np.full(cap + guard, 0xA5, np.uint8)
        off = np.zeros(4, np.uint64)
        assert _encode(dst, cap, off, frames, 0, 0, 3, 50, 33, 100) == 0
        assert off.tolist() == [0] + ends, cap
        fit = max([0] + [e for e in ends if e <= cap])
        assert dst[:fit].tobytes() == b"".join(want)[:fit], cap
        assert (dst[fit:] == 0xA5).all(), cap   # the frames that do not fit, and the guard bytes
    with pytest.raises(api.OpkError, match="need %d bytes, the buffer holds %d" % (ends[2], ends[1])):
        host.encode_jpeg(frames, 100, capacity=ends[1])
    assert host.encode_jpeg(frames, 100, capacity=ends[2]).tobytes_list() == want
    empty = host.encode_jpeg(np.zeros((0, 33, 50, 3), np.uint8), 100)
    assert empty.offsets.tolist() == [0] and empty.tobytes_list() == []


def test_save_names_the_files_as_the_reference_does(host, tmp_path):
    frames = np.stack([jc.gradient(34, 18), jc.noise(34, 18, 2)])
    batch = host.encode_jpeg(frames, 90)
    want = [jc.encode(f, 90) for f in frames]
    paths = batch.save(str(tmp_path / "images"), ["video_000000000000", "b"])
    assert [os.path.basename(p) for p in paths] == ["video_000000000000_rendered.jpg", "b_rendered.jpg"]
    assert [open(p, "rb").read() for p in paths] == want
    paths = batch.save(str(tmp_path / "video"), first_index=41)
    assert [os.path.basename(p) for p in paths] == ["000000000041_rendered.jpg",
                                                    "000000000042_rendered.jpg"]
    assert [open(p, "rb").read() for p in paths] == want
    with pytest.raises(ValueError):
        batch.save(str(tmp_path), ["one"])
    with pytest.raises(ValueError):
        batch.save(str(tmp_path))
    try:
        from PIL import Image
    except ImportError:
        return
    for p in paths:
        with Image.open(p) as im:
            assert im.size == (34, 18) and im.format == "JPEG"
            im.load()
    # and the decoded picture is the frame, to JPEG's accuracy at this quality
    with Image.open(io.BytesIO(want[0])) as im:
        rgb = np.asarray(im.convert("RGB")).astype(int)
    assert np.abs(rgb[..., ::-1] - frames[0]).mean() < 6


# ---- the host code under AddressSanitizer / UBSan, as a plain program ------------------------------
def _host_compiler():
    rocm = os.path.join(os.path.dirname(os.path.realpath(opk_build.HIPCC)), "..")
    return os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "include")


def _lcg(count, seed):
    out, s = np.empty(count, np.uint8), seed & 0xFFFFFFFF
    for i in range(count):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = s >> 24
    return out


def test_host_code_under_sanitizers(tmp_path):
    cxx, hip_include = _host_compiler()
    if not os.path.exists(cxx):
        pytest.skip("no host compiler beside hipcc")
    exe = str(tmp_path / "jpeg_driver")
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + hip_include,
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "jpeg_driver.cpp"),
           os.path.join(ROOT, "openpose_amd", "csrc", "host", "jpeg.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "libclang_rt" in r.stderr:
        pytest.skip("sanitizer runtime missing")
    assert r.returncode == 0, r.stderr

    def run(*a):
        r = subprocess.run([exe] + [str(x) for x in a], capture_output=True, text=True, timeout=300)
        text = r.stdout + r.stderr
        assert "Sanitizer" not in text and "runtime error" not in text, text
        assert r.returncode == 0, text
        return r.stdout

    assert "sweep ok" in run("sweep")
    assert "bad ok" in run("bad")
    # and the program's file is the restatement's
    out = str(tmp_path / "f.jpg")
    run("file", 34, 18, 75, 5, out)
    im = _lcg(34 * 18 * 3, 5).reshape(18, 34, 3)
    assert open(out, "rb").read() == jc.encode(im, 75)
