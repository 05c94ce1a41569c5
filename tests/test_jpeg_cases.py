"""CPU: the numpy restatement of the JPEG frames (tests/jpeg_cases.py) held to libjpeg-turbo -- to
Pillow where it imports, byte for byte at the edge sizes and qualities, and to the files Pillow
wrote that are committed under tests/golden/jpeg/ -- and the constant tables of
kernels/jpeg_tables.inc held to the DQT and DHT segments of those files."""
import io
import os
import re
import time

import numpy as np
import pytest

from tests import jpeg_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg")
INC = os.path.join(ROOT, "openpose_amd", "csrc", "kernels", "jpeg_tables.inc")


def pillow_file(bgr, quality):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    rgb = np.ascontiguousarray(bgr[..., ::-1])
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def contents(w, h):
    return [jc.noise(w, h, w * 1000 + h), jc.gradient(w, h), jc.flat(w, h, 77), jc.zrl_image(w, h)]


@pytest.mark.parametrize("size", jc.SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_pillow_at_quality_100(size):
    pytest.importorskip("PIL")
    for im in contents(*size):
        assert jc.encode(im, 100) == pillow_file(im, 100)


@pytest.mark.parametrize("quality", jc.QUALITIES_50x33)
def test_restatement_equals_pillow_at_every_quality(quality):
    pytest.importorskip("PIL")
    for im in contents(50, 33):
        assert jc.encode(im, quality) == pillow_file(im, quality)


def test_cases_equal_pillow_and_cover_what_they_claim():
    cases = jc.cases()   # asserts the coverage conditions
    assert {n for n, _, _ in cases} >= set(jc.GOLDEN)
    pytest.importorskip("PIL")
    for name, im, q in cases:
        assert jc.encode(im, q) == pillow_file(im, q), name


def test_restatement_equals_the_committed_files():
    cases = {n: (im, q) for n, im, q in jc.cases()}
    for name in jc.GOLDEN:
        im = np.load(os.path.join(GOLDEN, name + ".npy"))
        assert im.shape[0] <= 64 and im.shape[1] <= 64
        assert np.array_equal(im, cases[name][0]), name   # the builder still makes this input
        blob = open(os.path.join(GOLDEN, name + ".jpg"), "rb").read()
        assert jc.encode(im, cases[name][1]) == blob, name
        assert blob[:jc.HEADER_BYTES] == jc.header(im.shape[1], im.shape[0], cases[name][1])


def test_restatement_is_fast_enough():
    im = jc.noise(320, 192, 3)
    t = time.perf_counter()
    jc.encode(im, 100)
    assert time.perf_counter() - t < 2.0


# ---- the tables of the product against the files' segments -----------------------------------------
def inc_tables():
    text = open(INC).read()
    out = {}
    for name, body in re.findall(r"(kJpeg\w+)\[\d+\] = \{([^}]*)\}", text):
        out[name] = [int(v, 0) for v in re.findall(r"0x[0-9a-fA-F]+|\d+", re.sub(r"//[^\n]*", "", body))]
    return out


def segments(blob):
    """{DQT id: 64 zigzag values}, {DHT class << 4 | id: (bits, values)} of a file's header."""
    dqt, dht, i = {}, {}, 2
    while blob[i + 1] != 0xDA:
        assert blob[i] == 0xFF
        marker, length = blob[i + 1], (blob[i + 2] << 8) | blob[i + 3]
        seg = blob[i + 4:i + 2 + length]
        if marker == 0xDB:
            dqt[seg[0]] = list(seg[1:65])
        if marker == 0xC4:
            bits = list(seg[1:17])
            dht[seg[0]] = (bits, list(seg[17:17 + sum(bits)]))
            assert 17 + sum(bits) == len(seg)
        i += 2 + length
    return dqt, dht


def test_inc_tables_equal_the_files_segments():
    t = inc_tables()
    assert t["kJpegZigzag"] == jc.ZIGZAG and sorted(t["kJpegZigzag"]) == list(range(64))
    names = {0x00: "DC_LUMA", 0x10: "AC_LUMA", 0x01: "DC_CHROMA", 0x11: "AC_CHROMA"}
    cases = {n: (im, q) for n, im, q in jc.cases()}
    for name in jc.GOLDEN:
        q = cases[name][1]
        dqt, dht = segments(open(os.path.join(GOLDEN, name + ".jpg"), "rb").read())
        for tid, base in ((0, t["kJpegBaseLuma"]), (1, t["kJpegBaseChroma"])):
            scaled = jc.quant_table(base, q)
            assert dqt[tid] == [scaled[t["kJpegZigzag"][k]] for k in range(64)], (name, tid)
        assert sorted(dht) == sorted(names)
        for key, nm in names.items():
            assert dht[key] == (t["kJpegBits_" + nm], t["kJpegVals_" + nm]), (name, nm)
    # the restatement's own copies are the same constants
    assert t["kJpegBaseLuma"] == jc.BASE_LUMA and t["kJpegBaseChroma"] == jc.BASE_CHROMA
    for nm in names.values():
        assert t["kJpegBits_" + nm] == getattr(jc, "BITS_" + nm)
        assert t["kJpegVals_" + nm] == getattr(jc, "VALS_" + nm)
    # a quality-50 file carries the base tables themselves (Annex K.1, K.2)
    try:
        blob = pillow_file(jc.flat(8, 8, 0), 50)
    except pytest.skip.Exception:
        return
    dqt, _ = segments(blob)
    assert dqt[0] == [t["kJpegBaseLuma"][k] for k in t["kJpegZigzag"]]
    assert dqt[1] == [t["kJpegBaseChroma"][k] for k in t["kJpegZigzag"]]
