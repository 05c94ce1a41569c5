"""CPU: the host functions of the rotated and flipped frames -- opk_orient_size and
opk_orient_keypoints against the index map of the restatement (tests/orient_cases.py), every angle
the reference accepts and the ones it refuses, with its message text -- and the same host code with
the argument checks of opk_orient_frames under AddressSanitizer / UBSan in a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

from openpose_amd import _lib, api
from openpose_amd import build as opk_build
from tests import orient_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCEPTED = [r for r in range(-270, 361, 90)]   # -270 ... 360


def test_orient_size():
    for rotate in ACCEPTED + [450, -360, 720 + 90]:
        assert api.orient_size((7, 5), rotate) == oc.size(7, 5, rotate), rotate
    assert api.orient_size((7, 5), 90) == (5, 7) and api.orient_size((7, 5), -180) == (7, 5)
    assert api.orient_size((0, 0), 270) == (0, 0)
    with pytest.raises(api.OpkError, match="opk error 1"):
        api.orient_size((-1, 5), 0)


def grid_points(w, h):
    """Every pixel position of a w x h frame as keypoints [h, w, 3] with score 1."""
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs, ys, np.ones_like(xs)], -1).astype(np.float32)


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("rotate", ACCEPTED)
def test_keypoints_follow_the_index_map(rotate, flip):
    w, h = 7, 4
    src = grid_points(w, h)
    fwd = api.orient_keypoints(src, (w, h), rotate, flip)
    ow, oh = oc.size(w, h, rotate)
    # the oriented sample at fwd[sy, sx] is the source sample (sx, sy)
    x, y = fwd[..., 0].astype(int), fwd[..., 1].astype(int)
    assert np.array_equal(fwd[..., :2], np.stack([x, y], -1)) and (fwd[..., 2] == 1).all()
    assert x.min() == 0 and x.max() == ow - 1 and y.min() == 0 and y.max() == oh - 1
    qx, qy = oc.source_index(x, y, w, h, rotate, flip)
    assert np.array_equal(qx, src[..., 0].astype(int)) and np.array_equal(qy, src[..., 1].astype(int))
    # and the pixels agree: a frame whose samples name their own position
    names = (np.arange(h * w, dtype=np.int64).reshape(1, h, w, 1) % 251).astype(np.uint8)
    moved = oc.plane(names, rotate, flip)[0, :, :, 0]
    assert np.array_equal(moved[y, x], names[0, :, :, 0])
    # inverse undoes forward exactly, and is the restatement's map on the oriented grid
    assert np.array_equal(api.orient_keypoints(fwd, (w, h), rotate, flip, inverse=True), src)
    dst = grid_points(ow, oh)
    back = api.orient_keypoints(dst, (w, h), rotate, flip, inverse=True)
    sx, sy = oc.source_index(dst[..., 0].astype(int), dst[..., 1].astype(int), w, h, rotate, flip)
    assert np.array_equal(back[..., 0], sx.astype(np.float32))
    assert np.array_equal(back[..., 1], sy.astype(np.float32))


def test_keypoints_arithmetic_and_missing_points():
    """One fp32 subtraction from (float)(w - 1) or (float)(h - 1), or a copy; score 0 untouched."""
    w, h = 1280, 720
    kp = np.array([[[100.25, 7.5, 0.9], [0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [1279.0, 719.0, 1e-9]]],
                  np.float32)
    got = api.orient_keypoints(kp, (w, h), 90, 0)
    f = np.float32
    assert got[0, 0].tolist() == [f(7.5), f(1279.0) - f(100.25), f(0.9)]
    assert np.array_equal(got[0, 1], kp[0, 1]) and np.array_equal(got[0, 2], kp[0, 2])
    assert got[0, 3].tolist() == [f(719.0), f(0.0), f(1e-9)]
    got = api.orient_keypoints(kp, (w, h), 180, 1)
    assert got[0, 0].tolist() == [f(100.25), f(719.0) - f(7.5), f(0.9)]
    assert np.array_equal(kp[0, 0], np.array([100.25, 7.5, 0.9], np.float32))   # a copy is returned
    # no people, no parts
    assert api.orient_keypoints(np.zeros((0, 25, 3), np.float32), (w, h), 270, 1).shape == (0, 25, 3)
    assert api.orient_keypoints(np.zeros((2, 0, 3), np.float32), (w, h), 270, 1).shape == (2, 0, 3)


def _error(fn):
    with pytest.raises(api.OpkError) as e:
        fn()
    assert "opk error 1" in str(e.value)
    return str(e.value)


def test_refused_angles_and_flips():
    kp = grid_points(3, 2)
    for rotate, r in ((45, 45), (91, 91), (-45, -45), (360 + 91, 91), (-405, -45)):
        text = "Rotation angle = %d != {0, 90, 180, 270} degrees." % r
        assert text in _error(lambda: api.orient_size((3, 2), rotate))
        assert text in _error(lambda: api.orient_keypoints(kp, (3, 2), rotate, 0))
    L = _lib.load()
    buf = np.ascontiguousarray(kp)
    p = buf.ctypes.data
    assert L.opk_orient_keypoints(p, 2, 3, 3, 2, 90, 2, 0) == 1
    assert L.opk_orient_keypoints(p, 2, 3, 3, 2, 90, -1, 0) == 1
    assert L.opk_orient_keypoints(p, 2, 3, 3, 2, 90, 0, 2) == 1
    assert L.opk_orient_keypoints(p, -1, 3, 3, 2, 90, 0, 0) == 1
    assert L.opk_orient_keypoints(p, 2, 3, 0, 2, 90, 0, 0) == 1
    assert L.opk_orient_keypoints(None, 2, 3, 3, 2, 90, 0, 0) == 1
    assert L.opk_orient_keypoints(None, 0, 3, 3, 2, 90, 0, 0) == 0
    assert np.array_equal(buf, kp)   # a refused call writes nothing


# ---- the host code under AddressSanitizer / UBSan, as a plain program ------------------------------
def _host_compiler():
    rocm = os.path.join(os.path.dirname(os.path.realpath(opk_build.HIPCC)), "..")
    return os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "include")


def test_host_code_under_sanitizers(tmp_path):
    cxx, hip_include = _host_compiler()
    if not os.path.exists(cxx):
        pytest.skip("no host compiler beside hipcc")
    exe = str(tmp_path / "orient_driver")
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + hip_include,
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "orient_driver.cpp"),
           os.path.join(ROOT, "openpose_amd", "csrc", "host", "orient.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "libclang_rt" in r.stderr:
        pytest.skip("sanitizer runtime missing")
    assert r.returncode == 0, r.stderr

    def run(*a):
        r = subprocess.run([exe] + [str(x) for x in a], capture_output=True, text=True, timeout=120)
        text = r.stdout + r.stderr
        assert r.returncode in (0, 1), text
        assert "Sanitizer" not in text and "runtime error" not in text, text
        return r.returncode, r.stdout

    extremes = [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 90, -2 ** 31 + 88]
    for rotate in list(range(-450, 451, 45)) + [1, 91, -1] + extremes:
        ok = oc.normalize(rotate) is not None
        rc, out = run("size", 7, 5, rotate)
        assert rc == (0 if ok else 1), (rotate, out)
        if ok:
            assert out.split() == [str(v) for v in oc.size(7, 5, rotate)]
        else:
            assert "!= {0, 90, 180, 270} degrees." in out
        for flip in (0, 1):
            for inverse in (0, 1):
                rc, out = run("keypoints", 2, 3, 7, 5, rotate, flip, inverse)
                assert rc == (0 if ok else 1), (rotate, out)
    # the values, once: (90, 0) forward on points (1, 2, 0), (11, 12, 1), (21, 22, 2) of a 40 x 30 frame
    rc, out = run("keypoints", 1, 3, 40, 30, 90, 0, 0)
    assert rc == 0 and out.split()[:9] == ["1", "2", "0", "12", "28", "1", "22", "18", "2"]
    # 0 people, 0 parts, zero and negative sizes, bad flips
    assert run("keypoints", 0, 3, 7, 5, 90, 0, 0)[0] == 0
    assert run("keypoints", 3, 0, 7, 5, 90, 0, 0)[0] == 0
    assert run("keypoints", -1, 3, 7, 5, 90, 0, 0)[0] == 1
    assert run("keypoints", 2, 3, 0, 5, 90, 0, 0)[0] == 1
    assert run("keypoints", 2, 3, 7, -5, 90, 0, 0)[0] == 1
    assert run("keypoints", 2, 3, 7, 5, 90, 2, 0)[0] == 1
    assert run("keypoints", 2, 3, 7, 5, 90, 0, 7)[0] == 1
    assert run("size", 0, 0, 90) == (0, "0 0\n")
    assert run("size", -1, 5, 90)[0] == 1
    # the frame checks: format (0 BGR, 1 NV12, 2 I420), n, source size, destination size
    for fmt in (0, 1, 2):
        assert run("check", fmt, 2, 8, 6, 6, 8, 90, 0)[0] == 0
        assert run("check", fmt, 2, 8, 6, 8, 6, 180, 1)[0] == 0
        assert run("check", fmt, 0, 8, 6, 6, 8, -90, 1)[0] == 0       # n == 0 is no error
        assert run("check", fmt, 2, 8, 6, 8, 6, 90, 0)[0] == 1        # not the oriented size
        assert run("check", fmt, 2, 8, 6, 6, 8, 0, 0)[0] == 1
        assert run("check", fmt, 2, 0, 0, 0, 0, 0, 0)[0] == 1         # no area
        assert run("check", fmt, 2, 8, 0, 0, 8, 90, 0)[0] == 1
        assert run("check", fmt, -1, 8, 6, 6, 8, 90, 0)[0] == 1
        assert run("check", fmt, 2, 8, 6, 6, 8, 45, 0)[0] == 1
        assert run("check", fmt, 2, 8, 6, 6, 8, 90, 2)[0] == 1
    assert run("check", 7, 2, 8, 6, 6, 8, 90, 0)[0] == 1              # unknown format
    assert run("check", 1, 2, 7, 6, 6, 7, 90, 0)[0] == 1              # odd YUV width
    assert run("check", 0, 2, 7, 5, 5, 7, 270, 1)[0] == 0             # odd BGR sizes are frames
