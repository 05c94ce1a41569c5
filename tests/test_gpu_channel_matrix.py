"""GPU: the per-launch bound of tests/launch_check.py (every element of every launch against the
reference of the same operation fed with the GPU's own input blob; every concat slice against its
member's own blob, bit for bit) at output channel counts off the grid of the shipped pose models --
tests/channel_matrix_cases.py lists the graphs, the shapes and what each reaches.

Every case first asserts from the launch log that the instantiation it exists for ran
(tests/test_channel_matrix_plan.py asserts the same of the planner on the CPU), then runs the
checker on frames {first, last} with the project's constants (C_ACC, C_ACC_CHAINED, C_SPLIT) and
records max_frac_of_bound.  The small-batch cases also assert the mode's contract: every readable
blob and net_output are the bits of the same forward with the mode off.
"""
import numpy as np
import pytest

from tests import prototxt
from tests.channel_matrix_cases import (first_cases, head_cases, head_log_prefix, instantiation, odd_cases,
                                        offgrid_cases, offgrid_small_cases, pool_cases)
from tests.launch_check import check_concat_slices, check_launches, conv_instantiations, random_params
from tests.test_gpu_launch_matrix import every_conv_once, forwarded, image, report
from tests.test_gpu_small_batch import forwarded as forwarded_small
from tests.test_gpu_small_batch import readable_blobs

pytestmark = pytest.mark.gpu


def ids(cases):
    return dict(argvalues=cases, ids=[c["name"] for c in cases])


def assert_ran(log, case, graph):
    """The launch log shows every conv once, and the instantiations the case exists for."""
    every_conv_once(log, graph)
    ran = conv_instantiations(log, list(case["must_run"]))
    for name, prefix in case["must_run"].items():
        if prefix is None:   # inside the kernel of the conv before it
            assert len(ran[name]) == 1 and ran[name][0].startswith("conv_head_kernel<"), (name, log)
            continue
        assert len(ran[name]) == 1 and instantiation(ran[name][0], prefix, case["split"]), (name, prefix, log)
    return ran


def run_case(ctx, record_property, case, seed):
    """One forward of the case under LAUNCH_LOG=1 (small-batch cases: the mode off first), the
    instantiations asserted, every launch and every concat slice checked.  Returns (launch log,
    checker rows, layer list)."""
    L = case["graph"](*case["args"])
    graph = prototxt.parse(prototxt.emit(L))
    params = random_params(graph, seed)
    n, h, w = case["shape"]
    x = image(seed + 1, (n, 3, h, w))
    frames = sorted({0, n - 1})
    off = None
    if case["small"]:
        with forwarded_small(ctx, L, params, x, case["split"], False) as (net, log_off):
            assert not any(k.startswith("conv3s_kernel") for _, k in log_off), log_off
            off = readable_blobs(net, graph)
            off["net_output"] = net.output_numpy()
        run = forwarded_small(ctx, L, params, x, case["split"], True)
    else:
        run = forwarded(ctx, L, params, x, split=case["split"])
    with run as (net, log):
        assert_ran(log, case, graph)
        rows = check_launches(net, graph, params, x, frames, split=case["split"], log=log)
        if off is not None:
            on = readable_blobs(net, graph)
            on["net_output"] = net.output_numpy()
    if off is not None:   # the mode's contract: the same bits
        assert sorted(on) == sorted(off)
        for name in off:
            assert np.abs(off[name]).max() > 0, name
            np.testing.assert_array_equal(on[name], off[name], err_msg=name)
    report(record_property, case["name"], rows)
    return log, rows, L


# ---- 1: off-grid outputs ------------------------------------------------------------------------

@pytest.mark.parametrize("case", **ids(offgrid_cases()))
def test_offgrid_outputs(ctx, record_property, case):
    log, rows, _ = run_case(ctx, record_property, case, 201)
    assert [r.layer for r in rows] == ["c1", "c2", "c3", "c4", "c5", "c6", "c7", "c8", "c9"]
    convk = [k for _, k in log if k.startswith("conv")]
    assert all(("split" in k) == case["split"] for k in convk), convk


# ---- 2: the same graph on the small-batch tiles --------------------------------------------------

@pytest.mark.parametrize("case", **ids(offgrid_small_cases()))
def test_offgrid_outputs_small_batch(ctx, record_property, case):
    run_case(ctx, record_property, case, 203)


# ---- 3: odd concats and 7x7 ----------------------------------------------------------------------

@pytest.mark.parametrize("case", **ids(odd_cases()))
def test_odd_concats_and_7x7(ctx, record_property, case):
    log, rows, L = run_case(ctx, record_property, case, 205)
    # (run_case's check_launches compared the slices of these two concats: `a` in cat and cat2,
    # `c` in cat and cat2 next to its own buffer, and b and d trivially)
    assert [l["bottom"] for l in L if l["type"] == "Concat" and l["name"] != "net_output"] == \
        [["a", "b", "c"], ["d", "a", "c"]]
    assert sorted(r.layer for r in rows) == ["a", "b", "c", "c1", "d", "e", "f"]


def test_odd_concat_slices_are_compared(ctx):
    """The slice check on real kernels: six (concat, member) pairs, and the blobs it compares are
    different buffers where the member has more than one placement -- `c` read through its own
    buffer is the same bits as both of its concat slices, at the unaligned offsets 57 and 119."""
    case = odd_cases()[0]
    L = case["graph"]()
    graph = prototxt.parse(prototxt.emit(L))
    params = random_params(graph, 205)
    x = image(206, (2, 3, 24, 40))
    with forwarded(ctx, L, params, x) as (net, log):
        assert check_concat_slices(net, graph, [0, 1]) == 6
        cat, cat2, c, a = net.blob("cat"), net.blob("cat2"), net.blob("c"), net.blob("a")
    assert cat.shape[1] == 129 and cat2.shape[1] == 191
    assert np.abs(c).max() > 0 and np.abs(a).max() > 0
    np.testing.assert_array_equal(cat[:, 57:129], c)
    np.testing.assert_array_equal(cat2[:, 119:191], c)
    np.testing.assert_array_equal(cat[:, 0:19], a)
    np.testing.assert_array_equal(cat2[:, 100:119], a)


# ---- 4: fused heads ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", **ids(head_cases()))
def test_head_pairs(ctx, record_property, case):
    log, rows, _ = run_case(ctx, record_property, case, 207)
    n1, n2 = case["args"]
    fused = case["must_run"]["m7"] is None
    layers = [layer for layer, _ in log]
    if fused:
        assert layers == ["c1", "m6+m7"], log
        assert log[1][1].startswith(head_log_prefix(n1, n2)), log
        assert log[1][1].endswith(",split>") == case["split"], log
    else:
        assert layers == ["c1", "m6", "m7"], log
        assert not any(k.startswith("conv_head_kernel") for _, k in log), log


# ---- 5: the first conv ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", **ids(first_cases()))
def test_first_conv_outputs(ctx, record_property, case):
    log, rows, _ = run_case(ctx, record_property, case, 209)
    assert log[0][0] == "c1" and log[0][1].startswith("conv_image_kernel"), log
    assert rows[0].layer == "c1" and rows[0].amax > 0


# ---- 6: a stand-alone pool of off-grid channels --------------------------------------------------

@pytest.mark.parametrize("case", **ids(pool_cases()))
def test_pool_of_offgrid_channels(ctx, record_property, case):
    log, rows, _ = run_case(ctx, record_property, case, 211)
    pools = [k for layer, k in log if layer == "pool"]
    assert pools == ["maxpool2_split_kernel" if case["split"] else "maxpool2_kernel"], log
    assert rows[-1].layer == "p1" and rows[-1].frac == 0 and rows[-1].amax > 0   # exact, ceil sizing
