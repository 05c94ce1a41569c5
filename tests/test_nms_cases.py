"""The dense and tiny NMS cases (tests/nms_cases.py) contain what they claim, proved with the oracle
alone, and nmsGpu's restatement (oracle/nms.c orc_nms_cuda) gives the answers its source prescribes
on dense and tiny maps (nmsBase.cu:50-90,161-240).

The GPU test (tests/test_gpu_nms_dense.py) compares the kernels with the oracle on these inputs;
the preconditions here keep it from passing on an input that never reaches the path it is for:
the candidate sort and truncation (128-1024 peaks per plane), the ordered re-scan (more than
kNmsCandidates = 1024) and the columns where the two rule sets disagree.
"""
import numpy as np
import pytest

import oracle
from tests import nms_cases as nc

f32 = np.float32
RULES = [pytest.param(True, id="cuda"), pytest.param(False, id="cpu")]
# dense inputs: name -> [frames, 25, H, W] planes under the rule set
DENSE = {"A2": lambda cuda: nc.a2(), "A3": lambda cuda: nc.a3(), "A5": lambda cuda: nc.a5(),
         "B1": lambda cuda: nc.heat("B1", cuda), "B2": lambda cuda: nc.heat("B2", cuda),
         "B5": lambda cuda: nc.heat("B5", cuda)}
LANES = 256   # nms_finalize_kernel's workgroup: the candidate sort strides over more keys than this


def _counts(planes, cuda):
    return np.stack([nc.counts(fr, cuda) for fr in planes])


# ---- preconditions -------------------------------------------------------------------------------
@pytest.mark.parametrize("cuda", RULES)
@pytest.mark.parametrize("name", ["A2", "B1"])
def test_sorted_cases_hold_128_to_1024_peaks(name, cuda):
    c = _counts(DENSE[name](cuda), cuda)
    print("%s %s: %d-%d peaks per plane" % (name, "cuda" if cuda else "cpu", c.min(), c.max()))
    assert c.shape[1] == nc.PARTS and c.min() >= nc.CAP1 and c.max() <= nc.CANDIDATES
    assert c.max() <= LANES   # (as the issue measured them: one stride of the sort)


@pytest.mark.parametrize("cuda", RULES)
@pytest.mark.parametrize("name", ["A5", "B5"])
def test_strided_sort_cases_hold_257_to_1024_peaks(name, cuda):
    """The sorted cases above stay below 256 peaks, one key per lane of the finalize workgroup;
    these two give every plane more keys than lanes and fewer than the capacity: a sort network of
    512 or 1024 keys, two or four per lane."""
    c = _counts(DENSE[name](cuda), cuda)
    print("%s %s: %d-%d peaks per plane" % (name, "cuda" if cuda else "cpu", c.min(), c.max()))
    assert c.shape[1] == nc.PARTS and c.min() > LANES and c.max() <= nc.CANDIDATES


@pytest.mark.parametrize("cuda", RULES)
@pytest.mark.parametrize("name", ["A3", "B2"])
def test_rescan_cases_hold_more_than_1024_peaks(name, cuda):
    c = _counts(DENSE[name](cuda), cuda)
    print("%s %s: %d-%d peaks per plane" % (name, "cuda" if cuda else "cpu", c.min(), c.max()))
    assert c.shape[1] == nc.PARTS and c.min() > nc.CANDIDATES and c.max() < nc.FULL1 - 1


@pytest.mark.parametrize("cuda", RULES)
def test_mixed_batch_has_overflowing_and_sparse_planes(cuda):
    """A4: nearly every plane of frame 0 (A3 cropped to 100 x 100) overflows kNmsCandidates and
    leaves its counter above the capacity (the rest are sorted and truncated beside them); frame 1
    holds a few people."""
    c = _counts(nc.a4(), cuda)
    print("A4 %s: frame 0 %d-%d, frame 1 %d-%d" % ("cuda" if cuda else "cpu", c[0].min(), c[0].max(),
                                                   c[1].min(), c[1].max()))
    assert (c[0] > nc.CANDIDATES).sum() >= 20 and c[0].min() >= nc.CAP1
    assert c[1].max() < nc.CAP1 - 1 and c[1].sum() > 0


@pytest.mark.parametrize("kind", nc.TINY_KINDS)
@pytest.mark.parametrize("h,w", nc.TINY)
def test_tiny_maps_strict_interior(h, w, kind):
    """A1: no peak on a map without an interior, at most one per plane at 3 x 3; every peak the
    oracle reports is an interior pixel."""
    f = nc.tiny(h, w, kind)
    c = nc.counts(f, True)
    if h < 3 or w < 3:
        assert not c.any()
    if (h, w) == (3, 3):
        assert c.max() <= 1
    m = nc.peak_mask(f, True)
    np.testing.assert_array_equal(m.sum(axis=(1, 2)), c)
    assert not m[:, [0, -1], :].any() and not m[:, :, [0, -1]].any()


def test_tiny_maps_have_peaks_somewhere():
    """the continuous fields give peaks on every size with an interior above 3 x 3, and the 3 x 3
    field gives its single peak on some plane"""
    assert nc.counts(nc.tiny(3, 3, "uniform"), True).sum() >= 1
    for h, w in nc.TINY:
        if h >= 3 and w >= 3 and (h, w) != (3, 3):
            assert nc.counts(nc.tiny(h, w, "uniform"), True).sum() >= 3, (h, w)


def test_narrow_map_rules_disagree_on_the_edge_columns():
    """B3 (40 x 48): both rule sets report peaks on columns 1 and W-2, and some plane has a nmsCpu
    peak on column 1 or W-2 (the >= rule on a plateau, or an outer-border row) at a pixel where
    nmsGpu's rules report none."""
    cpu = nc.peak_mask(nc.heat("B3", False)[0], False)
    gpu = nc.peak_mask(nc.heat("B3", True)[0], True)
    np.testing.assert_array_equal(cpu.sum(axis=(1, 2)), nc.counts(nc.heat("B3", False)[0], False))
    np.testing.assert_array_equal(gpu.sum(axis=(1, 2)), nc.counts(nc.heat("B3", True)[0], True))
    W = cpu.shape[2]
    assert (cpu.shape[1], W) == (40, 48)
    for m in (cpu, gpu):
        assert m[:, :, 1].any() and m[:, :, W - 2].any()
    only_cpu = cpu & ~gpu
    planes = [c for c in range(nc.PARTS) if only_cpu[c, :, 1].any() or only_cpu[c, :, W - 2].any()]
    print("planes with a nmsCpu-only peak on column 1 / W-2:", planes)
    assert len(planes) >= 1
    assert only_cpu[:, 2:-2, 1].any()       # the plateau: an inner row, so only >= against > differs


def test_sparse_batch_after_overflow_is_sparse():
    """B4: the batch that follows B2 on the same extractor stays far below the capacities"""
    for cuda in (False, True):
        c = _counts(nc.heat("B4", cuda), cuda)
        assert c.max() < 32 and c.min() >= 1
    assert nc.source("B4").shape == nc.source("B2").shape


def test_restated_pipeline_scale():
    """scaleNetToOutput of the cases' sizes: finite, above 1 (1280 x 720 is larger than every net
    size here), and the offset is half a net pixel in output pixels"""
    for name in nc.SOURCES:
        s = nc.scale_net_to_output(name)
        assert s > 1 and np.isfinite(s)
        assert nc.offset_of(s) == pytest.approx(0.5 / float(s), rel=1e-6)


# ---- truncation is a prefix ----------------------------------------------------------------------
@pytest.mark.parametrize("cuda", RULES)
@pytest.mark.parametrize("name", sorted(DENSE))
def test_truncation_is_a_prefix(name, cuda):
    """oracle.nms(..., 128) is the first 127 entries of the untruncated run and nothing else"""
    for fr in DENSE[name](cuda):
        full = oracle.nms(fr, nc.TH, nc.FULL1, nc.OFFSET, cuda=cuda)
        cut = oracle.nms(fr, nc.TH, nc.CAP1, nc.OFFSET, cuda=cuda)
        assert (full[:, 0, 0] > nc.CAP1 - 1).all()
        np.testing.assert_array_equal(cut[:, 0, 0], nc.CAP1 - 1)
        np.testing.assert_array_equal(cut[:, 1:], full[:, 1:nc.CAP1])
        # raster order: the refined positions stay within 3 pixels of the peak's row
        assert (np.diff(full[:, 1:nc.CAP1, 1], axis=1) > -6.0).all()


# ---- known answers for orc_nms_cuda --------------------------------------------------------------
def test_cuda_cap_keeps_the_first_in_raster_order():
    """writeResultKernel (nmsBase.cu:161-240): 20 isolated strict maxima, maxPeaks + 1 = 8: the
    first 7 in raster order, slot 0 holds 7."""
    f = np.zeros((1, 30, 40), f32)
    rng = np.random.default_rng(5)
    cells = [(4 + 5 * r, 4 + 7 * c) for r in range(5) for c in range(5)]
    pos = sorted(cells[i] for i in rng.permutation(25)[:20])
    for k, (y, x) in enumerate(pos):
        f[0, y, x] = 0.3 + 0.03 * ((7 * k) % 20)      # heights in no order
    p = oracle.nms(f, 0.05, 8, channels=1, cuda=True)[0]
    assert p[0, 0] == 7 and p[0, 1] == 0 and p[0, 2] == 0
    for k in range(7):
        y, x = pos[k]
        assert p[k + 1, 2] == f[0, y, x]
        np.testing.assert_allclose(p[k + 1, :2], [x, y], atol=1e-5)   # round(x s) / s
    assert oracle.nms(f, 0.05, 64, channels=1, cuda=True)[0, 0, 0] == 20


def test_cuda_3x3_centroid_is_the_fused_sum_over_the_whole_map():
    """A 3 x 3 map whose centre is the maximum: one peak, centroid over all nine pixels (the 7 x 7
    window clipped on all four sides), sums as fmaf; a float64 restatement agrees within 1e-6."""
    f = f32([[[0.11, 0.32, 0.27], [0.43, 0.91, 0.38], [0.09, 0.56, 0.21]]])
    p = oracle.nms(f, 0.05, 8, (0.25, 0.5), channels=1, cuda=True)[0]
    assert p[0, 0] == 1
    yy, xx = np.mgrid[0:3, 0:3]
    s = f[0].astype(np.float64)
    assert p[1, 0] == pytest.approx((xx * s).sum() / s.sum() + 0.25, abs=1e-6)
    assert p[1, 1] == pytest.approx((yy * s).sum() / s.sum() + 0.5, abs=1e-6)
    assert p[1, 2] == f32(0.91)
    # the same sums in float, each product-and-add rounded once (fmaf), dy outer and dx inner
    xa = ya = sa = f32(0)
    for y in range(3):
        for x in range(3):
            xa = f32(np.float64(x) * np.float64(f[0, y, x]) + np.float64(xa))
            ya = f32(np.float64(y) * np.float64(f[0, y, x]) + np.float64(ya))
            sa = f32(sa + f[0, y, x])
    np.testing.assert_array_equal(p[1, :2], f32([xa / sa + f32(0.25), ya / sa + f32(0.5)]))
    # non-positive scores are left out of the sums (nmsBase.cu: `if (score > 0)`)
    g = f.copy()
    g[0, 0, 0] = -0.5
    q = oracle.nms(g, 0.05, 8, channels=1, cuda=True)[0]
    s[0, 0] = 0
    assert q[1, 0] == pytest.approx((xx * s).sum() / s.sum(), abs=1e-6)


@pytest.mark.parametrize("n", [1, 2, 3, 9, 64])
def test_cuda_two_row_map_has_no_peak(n):
    f = np.random.default_rng(n).random((3, 2, n), dtype=f32) + f32(0.1)
    assert not oracle.nms(f, 0.05, 8, channels=3, cuda=True).any()
    assert not oracle.nms(f.transpose(0, 2, 1), 0.05, 8, channels=3, cuda=True).any()
