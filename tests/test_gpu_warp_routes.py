"""GPU parity: the frame warp (input.hip) on each of its six kernel routes, with padded rows,
misaligned source bases and per-image tables, bit-equal to the oracle's warpAffine restatement.

launch_cvmat_to_input stages a workgroup's x table, weights and source rows in LDS when they fit
64 KiB (16-byte loads when base, row step and frame step allow: a16), else reads them directly.
Every case here reads the route it exists for from the launch log before it compares values.
"""
import numpy as np
import pytest
import torch

import oracle
import oracle.extract as ox
from openpose_amd import synth
from openpose_amd.api import HAND, KeypointExtractor, Net, launch_log
from tests import cpm_graphs, prototxt
from tests.kernel_routes import ran

pytestmark = pytest.mark.gpu


def _frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _size(h, w, scale):
    return int(np.ceil(h * scale)), int(np.ceil(w * scale))


def _padded(frames, step, offset=0):
    """The frames in a device buffer with `step` bytes per row, starting `offset` bytes into it:
    a [n, h, step] uint8 view (its pad bytes hold 0xAA, which no result may show)."""
    n, h, w, _ = frames.shape
    rows = np.full((n, h, step), 0xAA, np.uint8)
    rows[:, :, :w * 3] = frames.reshape(n, h, w * 3)
    buf = torch.full((offset + rows.size + 16,), 0x55, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + rows.size].view(n, h, step)
    view.copy_(torch.from_numpy(rows))
    assert view.data_ptr() % 16 == offset % 16
    return view


def _run(ctx, frames, scale, net_hw, normalize=1, step=None, offset=0):
    """the net input of `frames` (numpy [n, h, w, 3]) and the kernel that made it"""
    n, h, w, _ = frames.shape
    out = torch.full((n, 3) + tuple(net_hw), float("nan"), device="cuda")
    if step is None and offset == 0:
        dev, width = torch.from_numpy(frames).cuda(), None
    else:
        dev, width = _padded(frames, step or w * 3, offset), w
    with launch_log() as log:
        ctx.cvmat_to_input(out, dev, scale, normalize, width=width)
    assert len(log) == 1
    return out.cpu().numpy(), log


def _check(got, frames, scale, net_hw, normalize=1):
    for f in range(frames.shape[0]):
        np.testing.assert_array_equal(
            got[f], oracle.cvmat_to_input(frames[f], scale, net_hw[1], net_hw[0], normalize),
            err_msg="frame %d" % f)


@pytest.mark.parametrize("w,scale,route", [(11000, 0.5, "cvmat_to_input<2>"),
                                           (5000, 1.25, "cvmat_to_input<4>")])
def test_direct_kernels(ctx, w, scale, route):
    """Frames too wide for the staged kernel: 11000 x 6 halved (linear) and 5000 x 6 enlarged by
    1.25 (cubic) run the direct kernels."""
    frames = _frames(2, 6, w, seed=w)
    net_hw = _size(6, w, scale)
    assert net_hw == ((3, 5500) if scale < 1 else (8, 6250))
    got, log = _run(ctx, frames, scale, net_hw)
    ran(log, route)
    _check(got, frames, scale, net_hw)


@pytest.mark.parametrize("scale,k", [(0.5, 2), (1.25, 4)])
def test_lds_boundary_widths(ctx, scale, k):
    """The widest frame that still takes the staged kernel and the next wider one (found from the
    launch log by bisection, rows padded to 16 bytes so that the staged route is the a16 one):
    both bit-equal to the oracle."""
    h = 6

    def route(w):
        frames = np.zeros((1, h, w, 3), np.uint8)
        _, log = _run(ctx, frames, scale, _size(h, w, scale), step=(w * 3 + 15) // 16 * 16)
        return log[0][1]

    lo, hi = 333, 11000 if k == 2 else 5000
    assert route(lo) == "cvmat_to_input_lds<%d,a16>" % k and route(hi) == "cvmat_to_input<%d>" % k
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if route(mid).startswith("cvmat_to_input_lds"):
            lo = mid
        else:
            hi = mid
    for w, want in ((lo, "cvmat_to_input_lds<%d,a16>" % k), (hi, "cvmat_to_input<%d>" % k)):
        frames = _frames(2, h, w, seed=w)
        net_hw = _size(h, w, scale)
        got, log = _run(ctx, frames, scale, net_hw, step=(w * 3 + 15) // 16 * 16)
        ran(log, want)
        _check(got, frames, scale, net_hw)


def test_odd_width_upscaled(ctx):
    """A 333-wide frame (999-byte rows: no 16-byte loads) enlarged: the cubic byte-load route."""
    frames = _frames(2, 40, 333, seed=3)
    net_hw = _size(40, 333, 1.3)
    got, log = _run(ctx, frames, 1.3, net_hw)
    ran(log, "cvmat_to_input_lds<4>")
    _check(got, frames, 1.3, net_hw)


@pytest.mark.parametrize("scale,k", [(0.75, 2), (1.5, 4)])
def test_padded_rows_and_misaligned_base(ctx, scale, k):
    """A row step of w * 3 + 5 (a cv::Mat step), and a base 1 byte into a larger buffer at an
    otherwise 16-byte-friendly step: the 16-byte loads turn themselves off (the log shows the byte
    route; the same frames at the aligned base take a16), values the oracle's, pad bytes unread."""
    frames = _frames(2, 16, 64, seed=10 + k)
    net_hw = _size(16, 64, scale)
    plain = "cvmat_to_input_lds<%d>" % k
    got, log = _run(ctx, frames, scale, net_hw, step=64 * 3 + 5)
    ran(log, plain)
    _check(got, frames, scale, net_hw)
    got, log = _run(ctx, frames, scale, net_hw, step=64 * 3 + 16)
    ran(log, "cvmat_to_input_lds<%d,a16>" % k)
    _check(got, frames, scale, net_hw)
    got, log = _run(ctx, frames, scale, net_hw, step=64 * 3 + 16, offset=1)
    ran(log, plain)
    _check(got, frames, scale, net_hw)
    got, log = _run(ctx, frames, scale, net_hw, step=64 * 3, offset=1)
    ran(log, plain)
    _check(got, frames, scale, net_hw)


@pytest.mark.parametrize("scale", [0.6, 1.7])
@pytest.mark.parametrize("net_w", [40, 129])
def test_canvas_larger_than_the_frame(ctx, scale, net_w):
    """A net input wider and taller than the scaled frame holds -0.5 (0 unnormalised) outside it;
    destination rows narrower than a wave (40) and of 129 (lanes stride the row)."""
    w = int(net_w / scale) - 9
    frames = _frames(2, 21, w, seed=net_w)
    sh, sw = _size(21, w, scale)
    net_hw = (sh + 7, net_w)
    assert sw + 4 < net_w
    for normalize in (1, 0):
        got, log = _run(ctx, frames, scale, net_hw, normalize)
        _check(got, frames, scale, net_hw, normalize)
        assert (got[:, :, sh + 2:, :] == (-0.5 if normalize else 0.0)).all()
        assert (got[:, :, :, sw + 2:] == (-0.5 if normalize else 0.0)).all()
        if not normalize:
            assert got.max() > 1.0 and (got == np.round(got)).all()


@pytest.mark.parametrize("h,w", [(40, 1921), (29, 31)])
def test_crop_tables_per_image(ctx, h, w):
    """The crop warp (one table pair per image, mirrored x table for left hands) on a frame wider
    than any crop and on one smaller than the net input: a mirrored left hand, rectangles wholly
    outside the frame to the right and above, and ordinary ones; every crop the oracle's."""
    graph = prototxt.parse(prototxt.emit(cpm_graphs.GRAPHS["builtin:HAND"]()))
    net = Net(ctx, "builtin:HAND")
    net.set_params(synth.he_weights(graph, seed=5, out_scale=0.05))
    ex = KeypointExtractor(ctx, net, HAND, (368, 368))
    frames = _frames(1, h, w, seed=h)
    s = float(min(h, w))
    rects = np.array([[[w * 0.3, 2.0, s * 0.8, s * 0.8], [w * 0.5 + 0.25, -3.5, s * 0.6, s * 0.6]],
                      [[w + 10.0, 1.0, s, s], [w * 0.2, -2 * s - 5, s, s]]], np.float32)
    with launch_log() as log:
        ex.forward(torch.from_numpy(frames).cuda(), rects)
    assert any(k.startswith("cvmat_to_input") for _, k in log)
    crops, mirrored = [], []
    for hand in range(2):
        for p in range(2):
            assert ox.hand_valid(rects[p, hand])
            crops.append(ox.hand_affine(rects[p, hand], 368, mirror=hand == 0))
            mirrored.append(hand == 0)
    got = ex.crops()
    assert len(got) == 4 and mirrored[0] and crops[0][0, 0] < 0   # the left hand's x runs backwards
    for (m, x), want in zip(got, crops):
        np.testing.assert_array_equal(m, want)
        np.testing.assert_array_equal(x, oracle.warp_affine_inv(frames[0], want, 368, 368))
    # person 1's rectangles: right of the frame (left hand, mirrored) and above it (right hand)
    assert (got[1][1] == -0.5).all() and (got[3][1] == -0.5).all()
    assert not (got[0][1] == -0.5).all() and not (got[2][1] == -0.5).all()
    ex.close()
