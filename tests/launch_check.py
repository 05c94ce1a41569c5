"""Per-launch checker shared by the GPU layer tests (test_gpu_layers.py, test_gpu_launch_matrix.py)
and its own CPU self-test (test_launch_check.py).

check_launches() takes a net after a forward under LAUNCH_LOG=1 and compares what every launch of
that forward wrote with the reference of the same operation fed with the net's OWN input blob of
that launch, element by element (never sampled):

  * conv units ("A", "A+pool", "A+B", "A+B+pool", oracle/fp16.py unit_from_launch): fp16 precision
    against the fp16-storage emulation (oracle/fp16.py), |gpu - ref| <= 2 ulp16(ref) + C S with
    C = C_ACC (one conv) or C_ACC_CHAINED (an fp16 intermediate kept on chip); split precision
    against the float64 conv of the hi + lo input (oracle/split.py), C = C_SPLIT.  Only the fp32
    summation order is left free, so a wrong lane, tap, bias, slope, pooling partner or a stale
    store cannot hide (tests/test_launch_check.py injects each of them);
  * heads whose only consumer is the net_output concat: their fp32 slice of net_output too (the
    concat offset);
  * every other destination of a conv (its slice of each concat it is a member of; blob() reads
    placement 0 only): the concat's slice equals the member's own blob bit for bit
    (check_concat_slices) -- the consumer of a concat is referenced to whatever the concat holds;
  * stand-alone pools (Pooling layers no conv unit of the log took into its epilogue): the output
    blob equals the max pool of the input blob exactly -- a max of fp16 values is exact, and in
    split precision the pooled hi + lo is the largest hi + lo of the window, exact in fp32.

The net only needs blob(name, (first frame, count)) and launch_log(): openpose_amd.api.Net, or the
emulated stand-in of the self-test.
"""
import collections

import numpy as np

from oracle import fp16 as emu
from oracle import split as sp

C_ACC = 2.0 ** -16          # one conv per kernel
C_ACC_CHAINED = 2.0 ** -14  # conv1_1 -> conv1_2 and Mconv6 -> Mconv7 inside one kernel
# split precision: fp32 accumulation + dropped lo*lo + weight residue (oracle/split.py); the worst
# launch measured 0.041 of 2^-16 (round 6, r6b), so 2^-19 keeps ~3x headroom -- a missing or
# misplaced pass (~2^-11 S) is 250x beyond it
C_SPLIT = 2.0 ** -19

# layer: the launch-log layer field (or the Pooling layer's name); kernel: the instantiation(s) that
# ran it; frac: worst |gpu - ref| / bound over the checked frames; ulp16: worst error in ulp16 where
# the output rounding dominates the bound (fp16 precision; 0 otherwise); amax: largest |ref|
Row = collections.namedtuple("Row", "layer kernel frac ulp16 amax")


def random_params(graph, seed):
    """He weights + non-zero biases + PReLU slopes in (0.05, 0.5) (all in [0, 1]: the max
    epilogue the bench runs)."""
    from openpose_amd import synth
    params = synth.he_weights(graph, seed=seed)
    rng = np.random.default_rng(seed + 1)
    out = {}
    for name, (w, b, s) in params.items():
        b = rng.normal(0.0, 0.05, b.shape).astype(np.float32)
        if s is not None:
            s = rng.uniform(0.05, 0.5, s.shape).astype(np.float32)
        out[name] = (w, b, s)
    return out


def _reference(u, x, params, split):
    """(ref, tol) of a unit for its input values x, float64 in split precision."""
    chained = len(u["convs"]) > 1
    if split:
        return sp.unit(u, x, params, C_SPLIT)
    return emu.unit(u, x, params, C_ACC_CHAINED if chained else C_ACC)


def _compare(what, layer, kernel, f, got, ref, tol, split):
    """Every element of got within tol of ref, or AssertionError naming the worst one.  Returns
    (fraction of the bound, ulp16 where the rounding dominates, max |ref|)."""
    assert got.shape == ref.shape, (layer, got.shape, ref.shape)
    d = np.abs(got.astype(np.float64) - ref) if split else np.abs(got - ref)
    bad = ~(d <= tol)   # (a NaN fails)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(np.isnan(d), np.inf, d - tol)), d.shape)
        raise AssertionError("%s (%s) frame %d: %d of %d elements beyond the %s; worst at %s: "
                             "gpu %r ref %r tol %r" % (layer, kernel, f, int(bad.sum()), d.size, what,
                                                       i, float(got[i]), float(ref[i]), float(tol[i])))
    ulps = 0.0
    if not split:   # in ulp16 where the output rounding dominates the bound (no cancellation)
        ulp = emu.ulp16(ref)
        dom = tol <= 3 * ulp
        ulps = float((d[dom] / ulp[dom]).max()) if dom.any() else 0.0
    return float((d / tol).max()), ulps, float(np.abs(ref).max())


def check_launches(net, graph, params, x, frames, split=False, log=None):
    """net: after a forward of the image batch x [n, 3, h, w] under LAUNCH_LOG=1 (log: its
    launch_log(), read here if None); graph / params: the net's layers and {conv: (w, b, slope)};
    frames: the frames to check; split: split precision.  Every distinct launch-log layer is
    checked once (frame runs log one layer several times).  Returns [Row]; raises AssertionError
    with layer, kernel, frame, index, GPU value, reference and bound."""
    log = net.launch_log() if log is None else log
    kernels = collections.OrderedDict()
    pool_kernels = []
    for layer, kernel in log:
        if layer == "pool":
            pool_kernels.append(kernel)
        elif kernel not in kernels.setdefault(layer, []):
            kernels[layer].append(kernel)
    bound = "split bound" if split else "bound"
    rows, units = [], {}
    for layer, ks in kernels.items():
        kernel = " ".join(ks)
        u = units[layer] = emu.unit_from_launch(graph, layer)
        worst = (0.0, 0.0, 0.0)
        for f in frames:
            xin = x[f:f + 1] if u["input"] == "image" else net.blob(u["input"], (f, 1))
            ref, tol = _reference(u, xin, params, split)
            got = net.blob(u["output"], (f, 1))   # (split: hi + lo; net_output heads: fp32)
            w = _compare(bound, layer, kernel, f, got, ref, tol, split)
            worst = tuple(max(a, b) for a, b in zip(worst, w))
        rows.append(Row(layer, kernel, *worst))

    # net_output (fp32): the slices of the heads that only the output concat reads, against the
    # reference from their own inputs
    out = [l for l in graph if l["type"] == "Concat" and l["top"][0] == "net_output"]
    if out:
        off = 0
        chans = {l["top"][0]: l["num_output"] for l in graph if l["type"] == "Convolution"}
        for b in out[0]["bottom"]:
            head = [lay for lay, u in units.items() if u["output"] == b and u["pool"] is None]
            assert len(head) == 1, (b, head)
            u = units[head[0]]
            if u["fp32_output"]:
                for f in frames:
                    ref, tol = _reference(u, net.blob(u["input"], (f, 1)), params, split)
                    got = net.blob("net_output", (f, 1))[:, off:off + ref.shape[1]]
                    _compare(bound + " (net_output slice)", head[0], " ".join(kernels[head[0]]), f,
                             got, ref, tol, split)
            off += chans[b]
        assert off == net.blob("net_output", (frames[0], 1)).shape[1], off

    check_concat_slices(net, graph, frames)

    # stand-alone pools: exact
    fused ={u["pool"]["name"] for u in units.values() if u["pool"] is not None}
    alone = [l for l in graph if l["type"] == "Pooling" and l["name"] not in fused]
    assert len(alone) == len(pool_kernels), ("pool launches", [l["name"] for l in alone], pool_kernels)
    for l, kernel in zip(alone, pool_kernels):
        amax = 0.0
        for f in frames:
            xin = net.blob(l["bottom"][0], (f, 1))
            got = net.blob(l["top"][0], (f, 1))
            ref = sp._maxpool64(xin.astype(np.float64), l["kernel_size"], l["stride"])
            assert got.shape == ref.shape, (l["name"], got.shape, ref.shape)
            bad = got.astype(np.float64) != ref
            if bad.any():
                i = np.unravel_index(np.argmax(bad), bad.shape)
                raise AssertionError("%s (%s) frame %d: %d of %d pooled elements differ from the max "
                                     "of the input blob; first at %s: gpu %r ref %r tol 0"
                                     % (l["name"], kernel, f, int(bad.sum()), bad.size, i,
                                        float(got[i]), float(ref[i])))
            amax = max(amax, float(np.abs(ref).max()))
        rows.append(Row(l["name"], kernel, 0.0, 0.0, amax))
    return rows


def check_concat_slices(net, graph, frames):
    """Every destination of a conv, not only its first: for every Concat but net_output and every
    member, the slice [off, off + ch) of the concat's blob holds the bits of the member's own blob
    (split precision: hi + lo of the same stored pair is the same float).  Trivially true where
    the member's only placement is that slice; a check of the second to sixth store of a conv that
    also has a buffer of its own or is a member of several concats.  Returns the number of
    (concat, member) pairs compared."""
    chans = {l["top"][0]: l["num_output"] for l in graph if l["type"] == "Convolution"}
    pairs = 0
    for l in graph:
        if l["type"] != "Concat" or l["top"][0] == "net_output":
            continue
        cat = l["top"][0]
        for f in frames:
            whole = np.ascontiguousarray(net.blob(cat, (f, 1)), np.float32)
            off = 0
            for b in l["bottom"]:
                own = np.ascontiguousarray(net.blob(b, (f, 1)), np.float32)
                assert own.shape[1] == chans[b], (b, own.shape, chans[b])
                part = np.ascontiguousarray(whole[:, off:off + chans[b]])
                assert part.shape == own.shape, (cat, b, part.shape, own.shape)
                bad = part.view(np.uint32) != own.view(np.uint32)
                if bad.any():
                    i = tuple(int(v) for v in np.unravel_index(np.argmax(bad), bad.shape))
                    raise AssertionError("%s (concat) member %s frame %d: %d of %d elements of the slice "
                                         "[%d, %d) differ from the member's own blob; first at %s: "
                                         "concat %r member %r tol 0"
                                         % (cat, b, f, int(bad.sum()), bad.size, off, off + chans[b], i,
                                            float(part[i]), float(own[i])))
                off += chans[b]
                pairs += f == frames[0]
            assert off == whole.shape[1], (cat, off, whole.shape)
    return pairs


def print_rows(rows, title=""):
    """The run output of a case: every checked launch, its instantiation and worst fraction of the
    bound."""
    if title:
        print(title)
    for r in rows:
        print("%-40s %-44s %.3f of bound  %.2f ulp16  |ref| <= %.3g" % r)


def conv_instantiations(log, names):
    """{conv name: [kernels]} of the launch-log entries that ran the named convs."""
    out = {n: [] for n in names}
    for layer, kernel in log:
        for c in layer.split("+"):
            if c in out:
                out[c].append(kernel)
    return out
