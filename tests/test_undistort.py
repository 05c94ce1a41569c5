"""CPU: the host functions of the undistortion -- opk_undistort_maps_host bit for bit against the
numpy restatement of the include/opk.h text (tests/undistort_cases.py), every argument error, the
reader of the calibration files (opk_camera_parameters_read) on the reference's example file and on
files the test writes, its error texts -- and the same host code under AddressSanitizer / UBSan in a
stand-alone program fed good, truncated and malformed files."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from openpose_amd import _lib, api
from openpose_amd import build as opk_build
from tests import undistort_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "camera_parameters")
W, H = 50, 37


def host_maps(K, dist, w=W, h=H):
    return api.Cameras([K], [dist], [(w, h)]).maps(0)


@pytest.mark.parametrize("name,dist,skew", [
    ("4", uc.D4_PINCUSHION, 0.0), ("5", uc.D5_BARREL, 0.0), ("8", uc.D8_EXAMPLE, 0.0),
    ("12", uc.D12, 0.0), ("5 with skew", uc.D5_BARREL, 0.37), ("k3 huge", uc.D5_K3_HUGE, 0.0),
    ("zero", np.zeros(4), 0.0)])
def test_maps_equal_the_restatement(name, dist, skew):
    K = uc.small_k(W, H, skew)
    m1, m2 = host_maps(K, dist)
    r1, r2 = uc.maps(K, dist, W, H)
    assert m1.dtype == r1.dtype and m2.dtype == r2.dtype
    assert np.array_equal(m1, r1) and np.array_equal(m2, r2), name


def test_host_pixel_by_hand_every_term():
    """The hand-worked pixel of tests/test_undistort_cases.py (all twelve coefficients non-zero)."""
    K = np.array([[100., 0., 50.], [0., 100., 40.], [0., 0., 1.]])
    dist = [0.2, 0.4, 0.02, 0.04, 0.8, 0.4, 0.8, 1.6, 0.01, 0.04, 0.03, 0.08]
    m1, m2 = host_maps(K, dist, 104, 92)
    assert m1[90, 100].tolist() == [97, 88] and m2[90, 100] == 4 * 32 + 4


def test_maps_of_the_example_lens_at_its_own_size():
    m1, m2 = host_maps(uc.K_EXAMPLE, uc.D8_EXAMPLE, 1280, 1024)
    r1, r2 = uc.maps(uc.K_EXAMPLE, uc.D8_EXAMPLE, 1280, 1024)
    assert np.array_equal(m1, r1) and np.array_equal(m2, r2)


def test_each_view_has_its_own_map():
    cams = api.Cameras([uc.small_k(W, H), uc.small_k(60, 40)], [uc.D8_EXAMPLE, uc.D4_PINCUSHION],
                       [(W, H), (60, 40)])
    for v, (K, d, w, h) in enumerate([(uc.small_k(W, H), uc.D8_EXAMPLE, W, H),
                                      (uc.small_k(60, 40), uc.D4_PINCUSHION, 60, 40)]):
        m1, m2 = cams.maps(v)
        r1, r2 = uc.maps(K, d, w, h)
        assert np.array_equal(m1, r1) and np.array_equal(m2, r2)


def _error(K, dist, size=(W, H)):
    with pytest.raises(api.OpkError) as e:
        api.Cameras([K], [dist], [size]).maps(0)
    return str(e.value)


def test_argument_errors():
    K = uc.small_k(W, H)
    bad = K.copy()
    bad[0, 2] = np.inf
    assert "opk error 1" in _error(bad, uc.D5_BARREL)
    bad = K.copy()
    bad[1, 1] = np.nan
    assert "opk error 1" in _error(bad, uc.D5_BARREL)
    assert "opk error 1" in _error(K, [0.1, np.inf, 0, 0])
    for n in (0, 1, 3, 6, 7, 9, 13):
        assert "opk error 1" in _error(K, np.zeros(n)), n
    assert "opk error 4" in _error(K, np.zeros(14))                # the tilted-sensor model
    singular = np.array([[100., 0., 50.], [0., 0., 40.], [0., 0., 1.]])
    assert "opk error 1" in _error(singular, uc.D5_BARREL)
    assert "opk error 1" in _error(np.zeros((3, 3)), uc.D5_BARREL)
    assert "opk error 1" in _error(K, uc.D5_BARREL, (0, H))
    assert "opk error 1" in _error(K, uc.D5_BARREL, (W, 0))
    # V < 1, NULL fields, a view outside the set: straight through the C ABI
    L = _lib.load()
    good = api.Cameras([K], [uc.D5_BARREL], [(W, H)])
    m1, m2 = np.zeros((H, W, 2), np.int16), np.zeros((H, W), np.uint16)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    s = good.struct()
    s.views = 0
    assert L.opk_undistort_maps_host(ctypes.byref(s), 0, p(m1), p(m2)) == 1
    s.views = -2
    assert L.opk_undistort_maps_host(ctypes.byref(s), 0, p(m1), p(m2)) == 1
    assert L.opk_undistort_maps_host(None, 0, p(m1), p(m2)) == 1
    s = good.struct()
    for view in (-1, 1):
        assert L.opk_undistort_maps_host(ctypes.byref(s), view, p(m1), p(m2)) == 1
    assert L.opk_undistort_maps_host(ctypes.byref(s), 0, None, p(m2)) == 1
    s.ncoef = None
    assert L.opk_undistort_maps_host(ctypes.byref(s), 0, p(m1), p(m2)) == 1
    assert not m1.any() and not m2.any()


# ---- the reader ----------------------------------------------------------------------------------------
def _matrix(name, a, dt="d", fmt="%.17g"):
    a = np.asarray(a)
    rows, cols = a.shape
    return ('<%s type_id="opencv-matrix">\n  <rows>%d</rows>\n  <cols>%d</cols>\n  <dt>%s</dt>\n'
            '  <data>\n    %s</data></%s>\n'
            % (name, rows, cols, dt, " ".join(fmt % v for v in a.reshape(-1)), name))


def _file(path, ext, K, dist, initial=None, dt="d", fmt="%.17g",
          head='<?xml version="1.0"?>\n<!-- a comment -->\n'):
    text = head + "<opencv_storage>\n" + _matrix("CameraMatrix", ext, dt, fmt) \
        + _matrix("Intrinsics", K, dt, fmt) + _matrix("Distortion", dist, dt, fmt)
    if initial is not None:
        text += _matrix("CameraMatrixInitial", initial, dt, fmt)
    with open(path, "w") as f:
        f.write(text + "</opencv_storage>\n")


def _extrinsics(seed):
    r = np.random.default_rng(seed)
    q, _ = np.linalg.qr(r.normal(size=(3, 3)))
    return np.concatenate([q, r.normal(size=(3, 1))], 1)


def test_reader_on_the_example_file():
    for cams in (api.CameraParameters.read(GOLDEN), api.CameraParameters.read(GOLDEN + "/", ["17012332"])):
        assert cams.serials == ["17012332"]
        assert np.array_equal(cams.intrinsics[0], uc.K_EXAMPLE)
        assert len(cams.distortions) == 1 and np.array_equal(cams.distortions[0], uc.D8_EXAMPLE)
        eye = np.eye(3, 4)
        assert np.array_equal(cams.extrinsics[0], eye)
        assert np.array_equal(cams.extrinsics_initial[0], eye)
        assert np.array_equal(cams.camera_matrices[0], np.concatenate([uc.K_EXAMPLE, np.zeros((3, 1))], 1))
        assert np.array_equal(cams.camera_matrices[0], api.camera_matrix(uc.K_EXAMPLE, eye))
    m1, _ = cams.cameras((1280, 1024)).maps(0)
    assert m1.shape == (1024, 1280, 2)


def test_reader_on_written_files(tmp_path):
    Ka, Kb = uc.small_k(640, 480), uc.small_k(800, 600, skew=0.25)
    Ea, Eb, Ei = _extrinsics(1), _extrinsics(2), _extrinsics(3)
    # sorted order is by name, not by creation: "b" is written first
    _file(tmp_path / "b_cam.xml", Eb, Kb, uc.D5_BARREL[None, :], initial=Ei)       # a 1 x 5 row vector
    _file(tmp_path / "a_cam.xml", Ea, Ka, uc.D12[:, None])                         # no initial matrix
    (tmp_path / "notes.txt").write_text("not a camera")
    (tmp_path / "c_cam.xml.example").write_text("not a camera either")
    (tmp_path / "D_CAM.XML").write_text("listed by no rule: only <serial>.xml is ever opened")
    cams = api.CameraParameters.read(tmp_path)
    assert cams.serials == ["a_cam", "b_cam"]
    assert np.array_equal(cams.intrinsics, np.stack([Ka, Kb]))
    assert np.array_equal(cams.extrinsics, np.stack([Ea, Eb]))
    assert np.array_equal(cams.distortions[0], uc.D12) and np.array_equal(cams.distortions[1], uc.D5_BARREL)
    assert np.array_equal(cams.extrinsics_initial, np.stack([np.eye(3, 4), Ei]))
    for v, (K, E) in enumerate(((Ka, Ea), (Kb, Eb))):
        assert np.array_equal(cams.camera_matrices[v], api.camera_matrix(K, E))
    # explicit serials: their order, and only them
    one = api.CameraParameters.read(tmp_path, ["b_cam"])
    assert one.serials == ["b_cam"] and np.array_equal(one.intrinsics[0], Kb)
    swapped = api.CameraParameters.read(tmp_path, ["b_cam", "a_cam"])
    assert swapped.serials == ["b_cam", "a_cam"] and np.array_equal(swapped.extrinsics[1], Ea)
    # the objects built from them
    tri = cams.triangulator((640, 480), min_views=2)
    assert tri.views == 2 and np.array_equal(tri.P, cams.camera_matrices)
    lens = cams.cameras([(640, 480), (800, 600)])
    assert lens.ncoef.tolist() == [12, 5]
    r1, r2 = uc.maps(Kb, uc.D5_BARREL, 800, 600)
    m1, m2 = lens.maps(1)
    assert np.array_equal(m1, r1) and np.array_equal(m2, r2)


def test_reader_float_files(tmp_path):
    K, E = uc.small_k(640, 480), _extrinsics(4)
    _file(tmp_path / "f.xml", E, K, uc.D5_BARREL[:, None], dt="f", fmt="%.9g")
    cams = api.CameraParameters.read(tmp_path, ["f"])
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    assert np.array_equal(cams.intrinsics[0], f32(K)) and np.array_equal(cams.extrinsics[0], f32(E))
    assert np.array_equal(cams.distortions[0], f32(uc.D5_BARREL))


def _read_error(directory, serials=None):
    with pytest.raises(api.OpkError) as e:
        api.CameraParameters.read(directory, serials)
    assert "opk error 1" in str(e.value)
    return str(e.value)


def test_reader_error_texts(tmp_path):
    K, E = uc.small_k(640, 480), np.eye(3, 4)
    tail = " of the camera with serial number `%s` (file: %s). Is its format valid? You might want " \
           "to check the example xml file."
    where = lambda s: tail % (s, os.path.join(str(tmp_path), s + ".xml"))
    full = _matrix("CameraMatrix", E) + _matrix("Intrinsics", K) + _matrix("Distortion", uc.D5_BARREL[:, None])
    parts = {"matrix": _matrix("CameraMatrix", E), "intrinsics": _matrix("Intrinsics", K),
             "distortion": _matrix("Distortion", uc.D5_BARREL[:, None])}
    for missing in parts:
        body = "".join(text for name, text in parts.items() if name != missing)
        (tmp_path / (missing + ".xml")).write_text("<opencv_storage>\n" + body + "</opencv_storage>\n")
        msg = _read_error(tmp_path, [missing])
        assert "Error at reading the camera %s parameters" % missing + where(missing) in msg
    assert "Error at reading the camera parameters" + where("absent") in _read_error(tmp_path, ["absent"])
    (tmp_path / "empty.xml").write_text("")
    assert "Error at reading the camera parameters" + where("empty") in _read_error(tmp_path, ["empty"])
    # malformed matrices name the file
    bad = {
        "count": full.replace("<rows>3</rows>\n  <cols>3</cols>", "<rows>4</rows>\n  <cols>3</cols>"),
        "number": full.replace(" 0 ", " 0x ", 1),
        "nodata": full.replace("<data>", "<dat>").replace("</data>", "</dat>"),
        "emptydata": _matrix("CameraMatrix", E) + _matrix("Intrinsics", K)
        + '<Distortion type_id="opencv-matrix"><rows>5</rows><cols>1</cols><dt>d</dt><data></data></Distortion>',
        "shape": _matrix("CameraMatrix", np.eye(3)) + _matrix("Intrinsics", K)
        + _matrix("Distortion", uc.D5_BARREL[:, None]),
        "six": _matrix("CameraMatrix", E) + _matrix("Intrinsics", K) + _matrix("Distortion", np.zeros((6, 1))),
        "dt": full.replace("<dt>d</dt>", "<dt>u</dt>", 1),
        "open": full.replace("</Intrinsics>", ""),
    }
    for name, body in bad.items():
        (tmp_path / (name + ".xml")).write_text("<opencv_storage>\n" + body + "</opencv_storage>\n")
        msg = _read_error(tmp_path, [name])
        assert os.path.join(str(tmp_path), name + ".xml") in msg, name
        assert "Error at reading" not in msg, name
    (tmp_path / "comment.xml").write_text("<!-- never closed\n<opencv_storage>" + full + "</opencv_storage>")
    assert "comment.xml" in _read_error(tmp_path, ["comment"])
    # the directory walk meets the bad files too; a missing directory is an argument error
    _read_error(tmp_path)
    _read_error(tmp_path / "nowhere")
    # 14 coefficients are read, and refused where the lenses are used
    _file(tmp_path / "good14.xml", E, K, np.zeros((14, 1)))
    cams = api.CameraParameters.read(tmp_path, ["good14"])
    assert cams.distortions[0].size == 14
    with pytest.raises(api.OpkError, match="opk error 4"):
        cams.cameras((640, 480)).maps(0)


# ---- the host code under AddressSanitizer / UBSan, as a plain program ------------------------------
def _host_compiler():
    llvm = os.path.join(os.path.dirname(os.path.realpath(opk_build.HIPCC)), "..", "lib", "llvm")
    return os.path.join(llvm, "bin", "clang++"), os.path.join(
        os.path.dirname(os.path.realpath(opk_build.HIPCC)), "..", "include")


def _clean(r):
    """The program ended by its own return (0 ok, 1 a library error), with no sanitizer report."""
    text = r.stdout + r.stderr
    assert r.returncode in (0, 1), text
    assert "Sanitizer" not in text and "runtime error" not in text, text
    return r.returncode, r.stdout


def test_host_code_under_sanitizers(tmp_path):
    cxx, hip_include = _host_compiler()
    if not os.path.exists(cxx):
        pytest.skip("no host compiler beside hipcc")
    exe = str(tmp_path / "undistort_driver")
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I" + hip_include, "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "undistort_driver.cpp"),
           os.path.join(ROOT, "openpose_amd", "csrc", "host", "undistort.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "libclang_rt" in r.stderr:
        pytest.skip("sanitizer runtime missing")
    assert r.returncode == 0, r.stderr
    run = lambda *a: subprocess.run([exe] + [str(x) for x in a], capture_output=True, text=True, timeout=120)

    # the maps: two views, the second asked for; bit for bit the restatement
    Ks = np.stack([uc.small_k(W, H), uc.small_k(61, 23, skew=0.37)])
    dist = np.zeros((2, 12))
    dist[0, :8], dist[1, :12] = uc.D8_EXAMPLE, uc.D12
    src, dst = tmp_path / "maps.in", tmp_path / "maps.out"
    for view, (w, h) in ((1, (61, 23)), (0, (W, H))):
        src.write_bytes(np.array([2, view], np.int32).tobytes() + Ks.tobytes() + dist.tobytes()
                        + np.array([8, 12], np.int32).tobytes() + np.array([W, H, 61, 23], np.int32).tobytes())
        assert _clean(run("maps", src, dst))[0] == 0
        raw = dst.read_bytes()
        m1 = np.frombuffer(raw[:w * h * 4], np.int16).reshape(h, w, 2)
        m2 = np.frombuffer(raw[w * h * 4:], np.uint16).reshape(h, w)
        r1, r2 = uc.maps(Ks[view], dist[view][:(8, 12)[view]], w, h)
        assert np.array_equal(m1, r1) and np.array_equal(m2, r2)
    # the k3 = 1e12 camera (values past int32 and NaN-free overflow) and a refused one
    dist[0] = 0
    dist[0, 4] = 1e12
    src.write_bytes(np.array([2, 0], np.int32).tobytes() + Ks.tobytes() + dist.tobytes()
                    + np.array([5, 12], np.int32).tobytes() + np.array([W, H, 61, 23], np.int32).tobytes())
    assert _clean(run("maps", src, dst))[0] == 0
    src.write_bytes(np.array([2, 0], np.int32).tobytes() + Ks.tobytes() + dist.tobytes()
                    + np.array([5, 14], np.int32).tobytes() + np.array([W, H, 61, 23], np.int32).tobytes())
    rc, out = _clean(run("maps", src, dst))
    assert rc == 1 and out.startswith("error 4")

    # the reader: the example file, written files, then truncated and malformed ones
    rc, out = _clean(run("read", GOLDEN))
    assert rc == 0 and out.splitlines()[-1] == "read ok"
    fields = out.splitlines()[0].split()
    assert fields[:3] == ["17012332", "8", "0"]
    assert [float(x) for x in fields[3 + 12:3 + 12 + 9]] == uc.K_EXAMPLE.reshape(-1).tolist()
    good = tmp_path / "good"
    good.mkdir()
    _file(good / "two.xml", _extrinsics(5), uc.small_k(640, 480), uc.D5_BARREL[None, :], initial=_extrinsics(6))
    _file(good / "one.xml", _extrinsics(7), uc.small_k(640, 480), uc.D12[:, None], dt="f", fmt="%.9g")
    rc, out = _clean(run("read", good))
    assert rc == 0 and [line.split()[0] for line in out.splitlines()[:2]] == ["one", "two"]
    assert _clean(run("read", good, "two"))[0] == 0
    text = (good / "two.xml").read_text()
    bad = tmp_path / "bad"
    bad.mkdir()
    cases = {
        "unterminated_tag": text.replace('<Intrinsics type_id="opencv-matrix">', "<Intrinsics type_id="),
        "unterminated_comment": text.replace("<!-- a comment -->", "<!-- a comment"),
        "rows_too_large": text.replace("<rows>3</rows>", "<rows>4000</rows>"),
        "rows_overflow": text.replace("<rows>3</rows>", "<rows>99999999999999999999</rows>"),
        "empty_data": text[:text.index("<data>") + 6] + text[text.index("</data>"):],
        "long_line": text.replace("<data>", "<data>" + "7" * (1 << 20), 1),
        "long_numbers": text.replace("<data>", "<data>" + "0. " * (1 << 18), 1),
        "no_close": text.replace("</opencv_storage>", ""),
        "cut_in_number": text[:text.index("<data>") + 20],
        "only_header": '<?xml version="1.0"?>',
        "open_pi": "<?xml version=",
        "nul_bytes": text.replace("<cols>", "<cols>\0", 1),
    }
    for cut in (1, 7, 40, len(text) // 3, len(text) // 2, len(text) - 30, len(text) - 3):
        cases["truncated_%d" % cut] = text[:cut]
    for name, body in cases.items():
        (bad / (name + ".xml")).write_text(body)
        rc, out = _clean(run("read", bad, name))
        assert rc == 1 and out.startswith("error 1"), (name, out[:200])
    assert _clean(run("read", bad))[0] == 1            # the walk over all of them
    assert _clean(run("read", tmp_path / "nowhere"))[0] == 1
