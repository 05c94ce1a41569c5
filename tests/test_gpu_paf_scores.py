"""GPU parity: the PAF line integrals, score by score, on every route of paf.hip.

The cases (tests/paf_cases.py: net outputs, hand-written peaks, thresholds; what they contain is
proved in tests/test_paf_cases.py) go through opk_paf_scores_sources, which builds the lazy heat map
with the pipeline's own function and launches the pipeline's kernels.  Every score of every
candidate line -- winners and losers alike -- is compared with the oracle's getScoreAB on the
oracle's merged map; every float the kernels must not write is checked against a sentinel; the
route the case exists for is read from the launch log and the staged bytes are asserted.

Bar: the values are equal as floats (np.testing.assert_array_equal; a line that passes the count
test with no sample is 0 / 0 = NaN on both sides -- the NaN's sign bit is the dividers' own and is
not compared).
"""
import numpy as np
import pytest
import torch

from openpose_amd.api import dev_switches, launch_log
from tests import paf_cases as pc
from tests.kernel_routes import ran

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF   # a NaN no arithmetic produces
ROUTE = {("dense", True, 1): "paf_dense<lds,spl>", ("dense", True, 0): "paf_dense<lds>",
         ("dense", False, 1): "paf_dense<spl>", ("dense", False, 0): "paf_dense",
         ("compact", True, 1): "paf_compact<lds,spl>", ("compact", True, 0): "paf_compact<lds>",
         ("compact", False, 1): "paf_compact<spl>", ("compact", False, 0): "paf_compact"}

_DEV = {}


def _dev(key, make):
    """device copies of the cases' inputs, uploaded once"""
    if key not in _DEV:
        v = make()
        _DEV[key] = [torch.from_numpy(a).cuda() for a in v] if isinstance(v, list) \
            else torch.from_numpy(v).cuda()
    return _DEV[key]


def _sentinel(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _launch(ctx, name, model, layout, spl, th, rec_floats=0):
    """(output as float32 numpy, staged bytes); asserts the route and the staged bytes"""
    g, t = pc.GEOMETRIES[name], pc.table(model)
    srcs = _dev(("src", name, model), lambda: pc.sources(name, model))
    pk = _dev(("peaks", name, model), lambda: pc.peaks(name, model))
    npairs = len(t["pairs"]) // 2
    out = _sentinel((pc.FRAMES, npairs, pc.MAX_PEAKS, pc.MAX_PEAKS) if layout == "dense"
                    else (pc.FRAMES, rec_floats))
    with dev_switches(PAF_SPL=spl), launch_log() as log:
        staged = ctx.paf_scores_sources(out, srcs, g["target"], pk, pose_model=model,
                                        inter_th=th[0], inter_min_above=th[1], nms_th=th[2],
                                        semantics=g.get("semantics", pc.MAPS_CPU),
                                        scale_ratios=g.get("ratios"), rec_floats=rec_floats)
    assert staged == g["staged"], "%s: %d bytes staged" % (name, staged)
    ran(log, ROUTE[(layout, staged > 0, spl)])
    assert len(log) == 1
    return out.cpu().numpy()


def _check_dense(got, name, model, th):
    t = pc.table(model)
    ref, pk = pc.reference(name, model, th), pc.peaks(name, model)
    for b in range(pc.FRAMES):
        written = np.zeros(got[b].shape, bool)
        for q in range(len(t["pairs"]) // 2):
            na, nb = pc.counts_of(pk[b], t, q)
            written[q, :na, :nb] = True
            np.testing.assert_array_equal(got[b, q, :na, :nb], ref[b][q, :na, :nb],
                                          err_msg="%s frame %d pair %d" % (name, b, q))
        assert (got[b].view(np.uint32)[~written] == SENTINEL).all(), "written outside nA x nB"


def _check_compact(got, name, model, th, fits=(True, True)):
    t = pc.table(model)
    ref, pk = pc.reference(name, model, th), pc.peaks(name, model)
    bits = got.view(np.uint32)
    for b in range(pc.FRAMES):
        if not fits[b]:
            assert got[b, 0] == -1.0 and (bits[b, 1:] == SENTINEL).all()
            continue
        want = pc.compact(ref[b], pk[b], t)
        assert got[b, 0] == float(len(want)) == float(pc.total_lines(pk[b], t))
        np.testing.assert_array_equal(got[b, 1:1 + len(want)], want,
                                      err_msg="%s frame %d" % (name, b))
        assert (bits[b, 1 + len(want):] == SENTINEL).all(), "written past the total"


def _rec_floats(name, model=pc.BODY_25, extra=17):
    t, pk = pc.table(model), pc.peaks(name, model)
    return max(pc.total_lines(pk[b], t) for b in range(pc.FRAMES)) + 1 + extra


@pytest.mark.parametrize("spl", [1, 0])
@pytest.mark.parametrize("layout", ["dense", "compact"])
@pytest.mark.parametrize("name", sorted(pc.GEOMETRIES))
def test_scores_every_route(ctx, name, layout, spl):
    """Every geometry, dense and compact, one sample per lane for the small pairs (PAF_SPL 1) and
    one line per lane throughout (0): all scores the oracle's, nothing else written, the route and
    the staged bytes as the case says."""
    th = pc.DEFAULT_TH
    if layout == "dense":
        _check_dense(_launch(ctx, name, pc.BODY_25, layout, spl, th), name, pc.BODY_25, th)
    else:
        got = _launch(ctx, name, pc.BODY_25, layout, spl, th, _rec_floats(name))
        _check_compact(got, name, pc.BODY_25, th)
        assert got[0, 0] != got[1, 0]   # the frames carry different totals


@pytest.mark.parametrize("spl", [1, 0])
@pytest.mark.parametrize("name", ["G1", "G4", "G6"])
def test_scores_threshold_sets(ctx, name, spl):
    """The connector thresholds off their defaults (inter_min_above 0.5, 0, 1, 1.5, -0.1; inter_th
    0 and -0.2; nms_th different from inter_th) on a staged, an unstaged and the exact-count
    geometry."""
    for th in pc.THRESHOLDS[1:]:
        got = _launch(ctx, name, pc.BODY_25, "compact", spl, th, _rec_floats(name))
        _check_compact(got, name, pc.BODY_25, th)


@pytest.mark.parametrize("th", [pc.DEFAULT_TH, pc.THRESHOLDS[-1]])
def test_g6_lines_at_the_count_threshold(ctx, th):
    """The eight G6 lines alone (n = 20 and 25, exactly n - 3 .. n passing samples; a 64-line pair,
    so each lane walks a staged line and may leave its loop early): 1 where the count reaches
    samples_needed, 0 one below it -- 19 / 20 against 0.95f included."""
    got = _launch(ctx, "G6", pc.BODY_25, "dense", 1, th)[0, pc.G6_PAIR]
    ref = pc.reference("G6", pc.BODY_25, th)[0][pc.G6_PAIR]
    lines = np.arange(8)
    want = [float(n - f >= pc.samples_needed(n, th[1]))
            for n, f in zip([20] * 4 + [25] * 4, pc.G6_FAILS)]
    assert 0.0 in want[:4] and 1.0 in want[:4] and 0.0 in want[4:] and 1.0 in want[4:]
    np.testing.assert_array_equal(ref[lines, lines], want)
    np.testing.assert_array_equal(got[lines, lines], want)


@pytest.mark.parametrize("spl", [1, 0])
def test_scores_materialised_map(ctx, spl):
    """G7: the materialised map of G1 (the oracle's) through opk_paf_scores."""
    th = pc.DEFAULT_TH
    hm = _dev(("heat", "G1"), lambda: np.stack(pc.heat("G1")))
    pk = _dev(("peaks", "G1", pc.BODY_25), lambda: pc.peaks("G1"))
    out = _sentinel((pc.FRAMES, 26, pc.MAX_PEAKS, pc.MAX_PEAKS))
    with dev_switches(PAF_SPL=spl), launch_log() as log:
        ctx.paf_scores(out, hm, pk)
    ran(log, ROUTE[("dense", False, spl)])
    _check_dense(out.cpu().numpy(), "G1", pc.BODY_25, th)


def test_scores_body_135(ctx):
    """BODY_135 (152 pairs, 135 parts) on G1, compact."""
    got = _launch(ctx, "G1", pc.BODY_135, "compact", 1, pc.DEFAULT_TH, _rec_floats("G1", pc.BODY_135))
    _check_compact(got, "G1", pc.BODY_135, pc.DEFAULT_TH)


@pytest.mark.parametrize("name", ["G1", "G3b"])
def test_compact_record_length(ctx, name):
    """A record one float short of frame 0's total + 1 reports -1 for that frame and writes nothing
    else to it (the shorter frame 1 still fits); one float more and it fits exactly."""
    t, pk = pc.table(), pc.peaks(name)
    total = [pc.total_lines(pk[b], t) for b in range(pc.FRAMES)]
    assert total[0] > total[1] + 1
    th = pc.DEFAULT_TH
    _check_compact(_launch(ctx, name, pc.BODY_25, "compact", 1, th, total[0]), name, pc.BODY_25,
                   th, fits=(False, True))
    _check_compact(_launch(ctx, name, pc.BODY_25, "compact", 1, th, total[0] + 1), name,
                   pc.BODY_25, th)
