"""GPU: kernels/nms.hip on dense and tiny planes under both rule sets, bit for bit against the oracle
(oracle.nms(..., cuda=...) on oracle.resize_merge / resize_merge_cuda).  The inputs and the oracle's
answers come from tests/nms_cases.py; tests/test_nms_cases.py proves on the CPU that every input
reaches the path it is here for.

A  materialised maps under nmsGpu's rules (OPK_MAPS_CUDA): maps with no or one interior pixel and
   centroid windows clipped on all sides; 128-1024 peaks per plane (candidate sort over one and
   over several strides, truncation to the first 127, two rounds of refine_peaks with the fused
   sums); more than 1024 (the ordered re-scan: refine_write's fused branch); a dense and a sparse
   frame in one call, then the sparse one alone on the same scratch.
B  lazy maps through the pose pipeline, every detect kernel: the same counts on values evaluated
   on the fly, a map narrower than one walk, and a sparse batch after an overflowing one.
C  two and three sources under the CUDA build's rules (the raw-frame path supplies
   scaleInputToNetInputs): heat_at_cuda's multi-source branch in the windowed kernel.
D  the injection path refuses multi-scale CUDA maps and stays usable.
"""
import numpy as np
import pytest
import torch

import oracle
from oracle import body25
from openpose_amd import synth
from openpose_amd._lib import OpkError
from openpose_amd.api import (MAPS_CPU, MAPS_CUDA, Net, PoseExtractor, dev_switches, launch_log,
                              scale_and_size)
from tests import nms_cases as nc
from tests.kernel_routes import ran

pytestmark = pytest.mark.gpu

RULES = [pytest.param(True, id="cuda"), pytest.param(False, id="cpu")]


def _dev(a):
    return torch.from_numpy(np.array(a, np.float32, order="C")).cuda()   # (a copy: the cases are read-only)


def _same(got, ref, what=""):
    """Bit for bit: the count, every slot, and zeros in the unused slots (nms_finalize_kernel)."""
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got[..., 0, 0], ref[..., 0, 0], err_msg="%s: counts" % what)
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=what)


def _nms(ctx, planes, cuda):
    """opk_nms of [frames, 25, h, w] into a buffer that holds no zeros"""
    peaks = torch.full((planes.shape[0], nc.PARTS, nc.CAP1, 3), -3.0, device="cuda")
    with launch_log() as log:
        ctx.nms(peaks, _dev(planes), nc.TH, nc.OFFSET, semantics=MAPS_CUDA if cuda else MAPS_CPU)
    ran(log, "nms_detect")
    return peaks.cpu().numpy()


# ---- A: materialised maps ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", nc.TINY_KINDS)
@pytest.mark.parametrize("h,w", nc.TINY)
def test_cuda_rules_tiny_maps(ctx, h, w, kind):
    f = nc.tiny(h, w, kind)
    got = _nms(ctx, f[None], True)[0]
    ref = oracle.nms(f, nc.TH, nc.CAP1, nc.OFFSET, cuda=True)
    if h < 3 or w < 3:
        assert not got[:, 0, 0].any()
    if (h, w) == (3, 3):
        assert got[:, 0, 0].max() <= 1
    _same(got, ref, "%dx%d %s" % (h, w, kind))


def test_cuda_rules_sorted_and_truncated(ctx):
    """A2: 149-169 peaks per plane, two frames: the first 127 in raster order"""
    got = _nms(ctx, nc.a2(), True)
    assert (got[:, :, 0, 0] == nc.CAP1 - 1).all()
    _same(got, nc.materialised_reference("a2", True), "A2")


@pytest.mark.parametrize("cuda", RULES)
def test_sort_over_more_keys_than_lanes(ctx, cuda):
    """A5: 531-572 peaks per plane: the 1024-key sort network, four keys per lane"""
    got = _nms(ctx, nc.a5(), cuda)
    assert (got[:, :, 0, 0] == nc.CAP1 - 1).all()
    _same(got, nc.materialised_reference("a5", cuda), "A5")


@pytest.mark.parametrize("cuda", RULES)
def test_overflow_rescan(ctx, cuda):
    """A3: more than 1024 peaks on every plane: refine_write, fused under nmsGpu's rules"""
    got = _nms(ctx, nc.a3(), cuda)
    assert (got[:, :, 0, 0] == nc.CAP1 - 1).all()
    _same(got, nc.materialised_reference("a3", cuda), "A3")


@pytest.mark.parametrize("cuda", RULES)
def test_mixed_batch_then_sparse_frame(ctx, cuda):
    """A4: an overflowing frame beside a sparse one, then the sparse one alone on the scratch the
    overflowing frame used (its counters were above the capacity)."""
    f, ref = nc.a4(), nc.materialised_reference("a4", cuda)
    _same(_nms(ctx, f, cuda), ref, "A4 both frames")
    _same(_nms(ctx, f[1:], cuda), ref[1:], "A4 sparse frame after the overflow")
    _same(_nms(ctx, f, cuda), ref, "A4 both frames again")


# ---- B: lazy maps through the pose pipeline ------------------------------------------------------
# id: (CUDA rules, dev switches, the detect route that must run)
MODES = {"cpu-walk2": (False, {}, "nms_detect_walk2<1,cold>"),
         "cpu-windowed": (False, dict(NMS_STREAM=0), "nms_detect_lazy"),
         "cpu-ring": (False, dict(NMS_WALK=0), "nms_detect_stream<1>"),
         "cuda": (True, {}, "nms_detect_lazy")}


def _extractor(ctx, cuda):
    pose = PoseExtractor(ctx, None)
    if cuda:
        pose.set_map_semantics(MAPS_CUDA)
    return pose


def _inject(pose, name, mode):
    """One batch of case `name` through forward_net_output; the route is read from the launch log
    before any value is compared.  Returns (peaks, the oracle's peaks, people of frame 0)."""
    cuda, switches, route = MODES[mode]
    dev = _dev(nc.source(name))
    with dev_switches(**switches), launch_log() as log:
        pose.forward_net_output(dev, nc.net_size(name), nc.PRODUCER)
    ran(log, route)
    s = pose.scale_net_to_output()
    assert s == nc.scale_net_to_output(name)
    got = pose.peaks_numpy()
    people = pose.keypoints(0)          # the connector on the truncated lists completes
    assert people[0].shape[1:] == (nc.PARTS, 3)
    return got, nc.lazy_reference(name, cuda, nc.offset_of(s)), people


@pytest.mark.parametrize("mode", sorted(MODES))
def test_lazy_sorted_and_truncated(ctx, mode):
    """B1: 184 x 248 maps (no multiple of 16, 62 or 122) with 138-166 peaks per plane"""
    pose = _extractor(ctx, MODES[mode][0])
    got, ref, _ = _inject(pose, "B1", mode)
    assert (ref[:, :, 0, 0] == nc.CAP1 - 1).all()
    _same(got, ref, "B1 " + mode)
    pose.close()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_lazy_sort_over_more_keys_than_lanes(ctx, mode):
    """B5: 360 x 456 maps with 498-557 peaks per plane: the 512- and 1024-key sort networks on
    candidates in the order the detect kernel's atomics gave them"""
    pose = _extractor(ctx, MODES[mode][0])
    got, ref, _ = _inject(pose, "B5", mode)
    assert (ref[:, :, 0, 0] == nc.CAP1 - 1).all()
    _same(got, ref, "B5 " + mode)
    pose.close()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_lazy_overflow_rescan(ctx, mode):
    """B2: 640 x 960 maps with more than 1900 peaks per plane: the re-scan on evaluated values"""
    pose = _extractor(ctx, MODES[mode][0])
    got, ref, _ = _inject(pose, "B2", mode)
    assert (ref[:, :, 0, 0] == nc.CAP1 - 1).all()
    _same(got, ref, "B2 " + mode)
    pose.close()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_lazy_map_narrower_than_a_walk(ctx, mode):
    """B3: 40 x 48 maps (one window in x, three in y for the 16-row kernel) with peaks on columns 1
    and W-2, where the rule sets disagree"""
    pose = _extractor(ctx, MODES[mode][0])
    got, ref, people = _inject(pose, "B3", mode)
    assert ref[:, :, 0, 0].min() >= 1
    _same(got, ref, "B3 " + mode)
    pose.close()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_lazy_sparse_batch_after_overflow(ctx, mode):
    """B4: B2's field, then a sparse field of the same shape on the same extractor: the oracle's
    peaks, and a fresh extractor's peaks and people"""
    pose = _extractor(ctx, MODES[mode][0])
    got, ref, _ = _inject(pose, "B2", mode)
    _same(got, ref, "B2 " + mode)
    got, ref, people = _inject(pose, "B4", mode)
    _same(got, ref, "B4 after B2, " + mode)
    fresh = _extractor(ctx, MODES[mode][0])
    got1, _, people1 = _inject(fresh, "B4", mode)
    _same(got, got1, "B4: used and fresh extractor")
    np.testing.assert_array_equal(people[0], people1[0])
    np.testing.assert_array_equal(people[1], people1[1])
    fresh.close()
    pose.close()


# ---- C: two and three CUDA sources through the raw-frame path ------------------------------------
def _body25(ctx, seed):
    net = Net(ctx, "builtin:BODY_25")
    net.set_params(synth.he_weights(body25.layers(), seed=seed, out_scale=0.02))
    return net


@pytest.mark.parametrize("n", [2, 3])
def test_cuda_rules_multi_source_raw_frames(ctx, n):
    """--scale_number n on raw frames with OPK_MAPS_CUDA: resizeAndAddAndAverageKernel's merge
    evaluated inside nms_detect_lazy, the finalize kernel and the PAF scorer; heat maps, peaks and
    people the oracle chain's on the same per-scale net outputs."""
    size, frames = (160, 90), 2
    ratios, net_sizes = scale_and_size(size, (-1, 128), 1.0, n, 0.25)
    W, H = net_sizes[0]
    net = _body25(ctx, 70 + n)
    pose = PoseExtractor(ctx, net)
    pose.set_map_semantics(MAPS_CUDA)
    pose.set_input((-1, 128), scale_number=n, scale_gap=0.25)
    raw = np.random.default_rng(80 + n).integers(0, 256, (frames, size[1], size[0], 3), dtype=np.uint8)
    # the overlay rides on scale 0 only: scaled so that the average over the scales keeps people
    ov = np.stack([synth.overlay(3, H // 8, W // 8, seed=2500 + 10 * n + k) for k in range(frames)])
    ov = (ov * np.float32(max(1.0, n / 4.0))).astype(np.float32)
    ovd = _dev(ov)
    pose.set_overlay(ovd)
    with launch_log() as log:
        pose.forward_frames(torch.from_numpy(raw).cuda())
    ran(log, "nms_detect_lazy")
    s = pose.scale_net_to_output()
    off = nc.offset_of(s)
    gpu_heat = pose.heatmaps_numpy()
    gpu_peaks = pose.peaks_numpy()
    people = [pose.keypoints(k) for k in range(frames)]
    xs = [pose.net_input_numpy(i) for i in range(n)]
    assert [x.shape[2:] for x in xs] == [(h, w) for (w, h) in net_sizes]
    outs = []
    for x in xs:                         # the per-scale net outputs, without the overlay
        net.forward(_dev(x))
        outs.append(net.output_numpy())
    assert gpu_heat.shape == (frames, 78, H, W)
    for k in range(frames):
        heat = oracle.resize_merge_cuda([outs[0][k] + ov[k]] + [o[k] for o in outs[1:]], H, W, ratios)
        np.testing.assert_array_equal(gpu_heat[k], heat)
        peaks = oracle.nms(heat, nc.TH, nc.CAP1, (off, off), cuda=True)
        assert peaks[:, 0, 0].sum() >= 1
        _same(gpu_peaks[k], peaks, "frame %d" % k)
        rk, rs = oracle.connect(heat, peaks, scale=s)
        np.testing.assert_array_equal(people[k][0], rk)
        np.testing.assert_array_equal(people[k][1], rs)
    pose.close()
    net.close()


# ---- D: refused inputs ---------------------------------------------------------------------------
def test_multi_scale_cuda_injection_is_refused(ctx):
    """forward_multi has no scaleInputToNetInputs: with OPK_MAPS_CUDA it raises, and the extractor
    still gives the oracle's peaks for the next batch."""
    net = _body25(ctx, 9)
    pose = PoseExtractor(ctx, net)
    pose.set_map_semantics(MAPS_CUDA)
    rng = np.random.default_rng(10)
    xs = [_dev(rng.uniform(-0.5, 0.5, (1, 3, h, w))) for h, w in ((64, 96), (32, 48))]
    with pytest.raises(OpkError, match="needs scaleInputToNetInputs"):
        pose.forward_multi(xs, (96, 64))
    assert pose.pending() == 0
    got, ref, _ = _inject(pose, "B3", "cuda")
    assert ref[:, :, 0, 0].min() >= 1
    _same(got, ref, "B3 after the refused batch")
    pose.close()
    net.close()
