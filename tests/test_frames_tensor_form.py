"""The tensor form of `frames` (openpose_amd/api._as_frames): what every frame-taking method asserts
of a tensor before it describes it as Frames.bgr -- uint8, [n, h, w, 3] (or [n, h, row bytes] with
`width` where padded rows are accepted), a contiguous CUDA tensor -- and a Frames left alone.
No GPU: every case fails, or passes, before a device pointer is taken."""
import pytest
import torch

from openpose_amd.api import FRAMES_NV12, Frames, _as_frames


def test_frames_pass_through():
    fr = Frames(FRAMES_NV12, [None, None], 2, 32, 4)
    assert _as_frames(fr) is fr and _as_frames(fr, rows=True) is fr


@pytest.mark.parametrize("rows", [False, True])
def test_wrong_dtype(rows):
    with pytest.raises(AssertionError):
        _as_frames(torch.zeros((2, 4, 6, 3), dtype=torch.float32), rows=rows)


@pytest.mark.parametrize("rows", [False, True])
def test_wrong_channel_count(rows):
    with pytest.raises(AssertionError):
        _as_frames(torch.zeros((2, 4, 6, 4), dtype=torch.uint8), rows=rows)


def test_wrong_rank():
    """[n, h, row bytes] is a shape only where padded rows are accepted (cvmat_to_input), and needs
    the width there; elsewhere the four sizes do not unpack."""
    t = torch.zeros((2, 4, 24), dtype=torch.uint8)
    with pytest.raises(ValueError):
        _as_frames(t)
    with pytest.raises(AssertionError, match="padded rows need the frame width"):
        _as_frames(t, rows=True)
    with pytest.raises(AssertionError, match="padded rows need the frame width"):
        _as_frames(t, width=9, rows=True)   # 27 bytes do not fit a row of 24
    with pytest.raises(AssertionError):
        _as_frames(torch.zeros((2, 4, 6, 3), dtype=torch.uint8), width=5, rows=True)
    with pytest.raises(AssertionError):
        _as_frames(torch.zeros((4, 6, 3, 1, 1), dtype=torch.uint8), rows=True)


@pytest.mark.parametrize("rows", [False, True])
def test_host_or_strided_tensor(rows):
    msg = "device tensors must be contiguous CUDA tensors"
    host = torch.zeros((2, 4, 6, 3), dtype=torch.uint8)
    with pytest.raises(AssertionError, match=msg):
        _as_frames(host, rows=rows)
    with pytest.raises(AssertionError, match=msg):
        _as_frames(torch.zeros((2, 4, 12, 3), dtype=torch.uint8)[:, :, ::2], rows=rows)
