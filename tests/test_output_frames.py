"""The output image on the CPU side: the argument checks of opk_cvmat_to_output /
opk_output_to_cvmat / opk_render_frames / opk_pose_render_frames on a host-only context (all of them
happen before any device work), and the known answers of OpOutputToCvMat's two casts as a numpy
restatement that tests/test_gpu_output_frames.py holds the kernels to.

  OPK_CAST_CPU   cv::Mat::convertTo(CV_8UC3) (opOutputToCvMat.cpp:77-130): saturate_cast<uchar>(
                 cvRound(v)) -- round to nearest, ties to even, then clamp to [0, 255];
  OPK_CAST_CUDA  uCharImageCast (gpu/cuda.cu:27-34): (uchar) fastTruncateCuda(v, 0, 255) -- clamp,
                 then truncate toward zero."""
import ctypes

import numpy as np
import pytest

from openpose_amd import _lib
from openpose_amd.api import CAST_CPU, CAST_CUDA, LAYER_FACE, LAYER_HAND, LAYER_POSE

OPK_ERR_ARG, OPK_ERR_STATE = 1, 3        # include/opk.h
OPK_MPI_15 = 2
assert (CAST_CPU, CAST_CUDA, LAYER_POSE, LAYER_FACE, LAYER_HAND) == (0, 1, 0, 1, 2)   # OPK_CAST_*, OPK_LAYER_*


def cast_restated(v, cast):
    """The two reference expressions on a float32 array."""
    v = np.asarray(v, np.float32)
    if cast == CAST_CPU:
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)       # cvRound, then saturate_cast
    return np.minimum(np.float32(255), np.maximum(np.float32(0), v)).astype(np.uint8)   # truncates


KNOWN = [(CAST_CPU, 0.5, 0), (CAST_CPU, 1.5, 2), (CAST_CPU, 2.5, 2), (CAST_CPU, 254.5, 254),
         (CAST_CPU, 255.5, 255), (CAST_CPU, 300, 255), (CAST_CPU, -0.4, 0), (CAST_CPU, -7, 0),
         (CAST_CUDA, 0.99, 0), (CAST_CUDA, 254.99, 254), (CAST_CUDA, 255.5, 255),
         (CAST_CUDA, -3, 0)]


@pytest.mark.parametrize("cast,value,want", KNOWN)
def test_cast_known_answers(cast, value, want):
    assert int(cast_restated([value], cast)[0]) == want


def _layer(kind=LAYER_POSE, counts=(1,), alpha=0.6, pose_model=0, googly=0, threshold=0.05):
    c = (ctypes.c_int * len(counts))(*counts)
    s = _lib.RenderLayerStruct(kind, pose_model, ctypes.c_void_p(64), c, threshold, alpha, googly)
    s._keep = c
    return s


def _layers(*ls):
    arr = (_lib.RenderLayerStruct * len(ls))(*ls)
    arr._keep = ls
    return arr


@pytest.fixture(scope="module")
def host():
    from openpose_amd.api import Context
    ctx = Context.host_only()
    yield ctx
    ctx.close()


def test_render_layer_struct_matches_header():
    """kind, pose_model, keypoints_dev, counts_host, render_threshold, alpha, googly_eyes -- the
    field order of opk_render_layer in include/opk.h."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "opk.h")).read()
    body = re.search(r"typedef struct opk_render_layer \{(.*?)\} opk_render_layer;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*(?=[,;])", body)
    assert names == [f[0] for f in _lib.RenderLayerStruct._fields_]


def test_output_abi_errors_host_only(host):
    L = host.L
    fake = ctypes.c_void_p(64)
    one = _layers(_layer())

    def frames(layers=one, n_layers=1, n=1, out=(64, 48), size=(64, 48), cast=CAST_CPU):
        return L.opk_render_frames(host.h, fake, 0, out[0], out[1], fake, n, size[0], size[1], 0,
                                   1.0, layers, n_layers, 1, cast)

    four = _layers(_layer(), _layer(LAYER_FACE), _layer(LAYER_HAND), _layer())
    cases = [
        (lambda: frames(out=(0, 48)), "Output resolution has 0 area."),
        (lambda: frames(out=(64, 0)), "Output resolution has 0 area."),
        (lambda: frames(size=(0, 48)), "Input images has 0 area."),
        (lambda: frames(_layers(_layer(alpha=1.5))), "Alpha must be in the range [0, 1]."),
        (lambda: frames(_layers(_layer(pose_model=OPK_MPI_15, googly=1))),
         "googlyEyes not compatible with MPI"),
        (lambda: frames(_layers(_layer(counts=(3, 128))), n=2), "POSE_MAX_PEOPLE = 127"),
        (lambda: frames(_layers(_layer(pose_model=15))), "Invalid Model."),
        (lambda: frames(cast=2), "cast"),
        (lambda: frames(four, 4), "at most 3 layers"),
        (lambda: L.opk_cvmat_to_output(host.h, fake, fake, 1, 64, 48, 0, 1.0, 0, 48),
         "Output resolution has 0 area."),
        (lambda: L.opk_cvmat_to_output(host.h, fake, fake, 1, 64, 0, 0, 1.0, 64, 48),
         "Input images has 0 area."),
        (lambda: L.opk_output_to_cvmat(host.h, fake, 0, fake, 1, 64, 48, 2), "cast"),
        (lambda: L.opk_output_to_cvmat(host.h, fake, 0, fake, 1, 0, 48, CAST_CPU),
         "Output resolution has 0 area."),
    ]
    for call, msg in cases:
        assert call() == OPK_ERR_ARG
        assert msg in L.opk_last_error().decode(), (msg, L.opk_last_error())
    # a face layer may hold 128 (up to 1024); the call then reaches the device work, which a
    # host-only context refuses with a state error: every argument check lies before it
    assert frames(_layers(_layer(LAYER_FACE, counts=(128,), threshold=0.4))) == OPK_ERR_STATE
    assert "host-only" in L.opk_last_error().decode()


def test_no_frames_is_success_without_device_work(host):
    L = host.L
    fake = ctypes.c_void_p(64)
    assert L.opk_render_frames(host.h, fake, 0, 64, 48, fake, 0, 64, 48, 0, 1.0, None, 0, 1,
                               CAST_CPU) == 0
    assert L.opk_render_frames(host.h, fake, 0, 64, 48, fake, 0, 64, 48, 0, 1.0,
                               _layers(_layer(counts=(0,))), 1, 1, CAST_CPU) == 0
    assert L.opk_cvmat_to_output(host.h, fake, fake, 0, 64, 48, 0, 0.5, 32, 24) == 0
    assert L.opk_output_to_cvmat(host.h, fake, 0, fake, 0, 64, 48, CAST_CUDA) == 0


def test_pose_render_frames_needs_a_collected_batch(host):
    from openpose_amd.api import PoseExtractor
    pose = PoseExtractor(host, net=None)
    fake = ctypes.c_void_p(64)
    rc = host.L.opk_pose_render_frames(pose.h, fake, 0, 64, 48, fake, 2, 64, 48, 0, 1.0, 0.05, 0.6,
                                       0, 1, CAST_CPU)
    assert rc == OPK_ERR_STATE
    assert "no collected batch" in host.L.opk_last_error().decode()
    pose.close()
