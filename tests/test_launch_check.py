"""CPU: the per-launch checker (tests/launch_check.py) accepts a correct net and rejects subtly
wrong kernels -- the evidence that the GPU tests built on it (test_gpu_layers.py,
test_gpu_launch_matrix.py) would fail on a wrong lane, tap, bias, slope, pooling partner, stale
store or missing split pass.

The checker is driven with a stand-in net (EmulatedNet) whose blob() and launch_log() are served
from an emulation of a small graph at 2 x 24 x 40 (conv 3 -> 64, conv 64 -> 64 + 2x2 pool,
conv 64 -> 96 PReLU, a 1x1 conv 96 -> 20, the inner concat of the two -- the 96-channel member at
offset 20, no multiple of 8, and with a reader of its own -- and a 1x1 head from the concat to the
fp32 net_output), in both precisions and with the pool in the conv's epilogue ("c2+pool") or as
its own launch.  The emulation evaluates every conv in float64
(torch) and rounds at the stores, so the clean stand-in differs from the checker's references
(oracle/fp16.py on the C oracle's fp32 sums; oracle/split.py) by what a correct kernel may differ
by -- the summation order and the stored pair's residue -- and must pass; each injected defect
must raise.
"""
import numpy as np
import pytest

from oracle import fp16 as emu
from oracle import split as sp
from tests import prototxt
from tests.launch_check import (C_ACC, C_ACC_CHAINED, C_SPLIT, check_concat_slices, check_launches,
                                random_params)

N, H, W = 2, 24, 40
DEFECTS = ["tap", "shift_x", "bias", "slope", "pool_partner", "stale_group"]


def graph4():
    def conv(name, bottom, cout, k, act=None):
        out = [dict(name=name, type="Convolution", bottom=[bottom], top=[name], num_output=cout,
                    kernel_size=k, pad=k // 2)]
        if act:
            out.append(dict(name=act + "_" + name, type="ReLU" if act == "relu" else "PReLU",
                            bottom=[name], top=[name]))
        return out
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", 64, 3, "relu")
    L.append(dict(name="p1", type="Pooling", bottom=["c2"], top=["p1"], kernel_size=2, stride=2))
    L += conv("c3", "p1", 96, 3, "prelu") + conv("c5", "c3", 20, 1)
    L.append(dict(name="cat", type="Concat", bottom=["c5", "c3"], top=["cat"]))
    L += conv("c4", "cat", 26, 1)
    L.append(dict(name="net_output", type="Concat", bottom=["c4"], top=["net_output"]))
    return prototxt.parse(prototxt.emit(L))


def _pair(v):
    """The value a split-precision blob holds: hi = fp16(v), lo = fp16(v - hi), read as hi + lo."""
    v = np.asarray(v, np.float32)
    hi = emu.f16(v)
    return hi + emu.f16(v - hi)


def _pool(x, wrong_partner):
    """2x2 / 2 max pool (even sizes); wrong_partner: the window takes column 2i + 2 for 2i + 1."""
    a, b = x[:, :, 0::2], x[:, :, 1::2]
    r = np.maximum(a, b)
    left = r[:, :, :, 0::2]
    right = r[:, :, :, 1::2]
    if wrong_partner:
        right = np.concatenate([left[:, :, :, 1:], right[:, :, :, -1:]], axis=3)
    return np.maximum(left, right)


class EmulatedNet:
    """blob() / launch_log() of a forward of graph4 as a correct kernel set would leave them,
    optionally with one defect."""

    def __init__(self, graph, params, x, split, fuse_pool, defect=None, runs=1):
        convs, _ = emu.annotate(graph)
        self.blobs = {}
        self.log = []
        cur = {"image": np.asarray(x, np.float32)}
        for l in graph:
            if l["type"] == "Convolution":
                c = convs[l["name"]]
                w, b, s = [None if a is None else np.array(a, np.float32) for a in params[l["name"]]]
                if defect == "tap" and l["name"] == "c3":
                    w[5, :, 0, 2] = 0          # one tap of one output channel
                if defect == "bias" and l["name"] == "c2":
                    b[7] = 0                   # bias dropped on one channel
                if defect == "slope" and l["name"] == "c3":
                    s[12] = s[11]              # channel 11's slope applied to channel 12
                xin = cur[l["bottom"][0]]
                if split:
                    if defect == "no_xlo_pass" and l["name"] == "c3":
                        xin = emu.f16(xin)     # x_lo w_hi omitted: only the hi half is read
                else:
                    xin, w = emu.f16(xin), emu.f16(w)
                t = sp._act64(sp._conv64(xin, w, b, c["pad"]), c["act"], s).astype(np.float32)
                if defect == "shift_x" and l["name"] == "c1":
                    t = np.roll(t, 1, axis=3)  # every output one pixel to the right
                fp32_out = l["name"] == "c4"
                v = t if fp32_out else (_pair(t) if split else emu.f16(t))
                if defect == "stale_group" and l["name"] == "c3":
                    v[N - 1, 8:16] = v[0, 8:16]   # one 8-channel group of the last frame not written
                cur[l["top"][0]] = v
                fused = fuse_pool and l["name"] == "c2"
                if not fused:
                    self.blobs[l["top"][0]] = v
                self.log += [(l["name"] + ("+pool" if fused else ""), "emulated<%s>" % l["name"])] * (
                    runs if l["name"] == "c3" else 1)
            elif l["type"] == "Pooling":
                cur[l["top"][0]] = self.blobs[l["top"][0]] = _pool(cur[l["bottom"][0]],
                                                                  defect == "pool_partner")
                if not fuse_pool:
                    self.log.append(("pool", "emulated_pool"))
            elif l["type"] == "Concat":
                v = np.concatenate([cur[b] for b in l["bottom"]], axis=1)
                if defect == "stale_concat_slice" and l["top"][0] == "cat":
                    # one 4-channel group of c3's slice (offset 20) of the last frame not written;
                    # c3's own buffer, which c5 reads, is right
                    v[N - 1, 20 + 8:20 + 12] = v[0, 20 + 8:20 + 12]
                cur[l["top"][0]] = self.blobs[l["top"][0]] = v

    def launch_log(self):
        return list(self.log)

    def blob(self, name, frames):
        f0, nf = frames
        if name not in self.blobs:
            raise RuntimeError(name + ": kept on chip by a fused kernel")
        return self.blobs[name][f0:f0 + nf].copy()


@pytest.fixture(scope="module")
def case():
    graph = graph4()
    params = random_params(graph, 71)
    x = np.random.default_rng(72).uniform(-0.5, 0.5, (N, 3, H, W)).astype(np.float32)
    return graph, params, x


def _run(case, split, fuse_pool, defect=None, runs=1):
    graph, params, x = case
    net = EmulatedNet(graph, params, x, split, fuse_pool, defect, runs)
    return check_launches(net, graph, params, x, [0, N - 1], split=split)


def test_constants_are_the_projects():
    """The bounds' constants, defined once (tests/launch_check.py) with the values the layer tests
    have used since they were set."""
    assert (C_ACC, C_ACC_CHAINED, C_SPLIT) == (2.0 ** -16, 2.0 ** -14, 2.0 ** -19)


@pytest.mark.parametrize("fuse_pool", [True, False])
@pytest.mark.parametrize("split", [False, True])
def test_clean_emulation_is_accepted(case, split, fuse_pool):
    """Every launch of the correct stand-in is within its bound; one row per distinct layer (a
    layer logged by three frame runs is checked once), the stand-alone pool as a row of its own."""
    rows = _run(case, split, fuse_pool, runs=3)
    layers = [r.layer for r in rows]
    assert layers == (["c1", "c2+pool", "c3", "c5", "c4"] if fuse_pool
                      else ["c1", "c2", "c3", "c5", "c4", "p1"])
    assert all(0 <= r.frac < 1 for r in rows)
    assert rows[2].kernel == "emulated<c3>"
    # the stand-in's float64 sums differ from the fp16 reference's fp32 sums: the check is not
    # comparing the reference with itself
    if not split:
        assert max(r.frac for r in rows) > 0
    if not fuse_pool:
        assert rows[-1].kernel == "emulated_pool" and rows[-1].frac == 0


@pytest.mark.parametrize("fuse_pool", [True, False])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("defect", DEFECTS)
def test_injected_defect_is_rejected(case, split, fuse_pool, defect):
    """One tap of one output channel zeroed, the output shifted by one pixel in x, the bias dropped
    on one channel, channel c's PReLU slope applied to c + 1, the pool taking the wrong partner
    column, one 8-channel group of one frame left stale: each raises, and the message names the
    layer, the kernel, the frame, the element, both values and the bound."""
    where = {"tap": "c3", "shift_x": "c1", "bias": "c2+pool" if fuse_pool else "c2", "slope": "c3",
             "pool_partner": "c2+pool" if fuse_pool else "p1", "stale_group": "c3"}[defect]
    with pytest.raises(AssertionError) as e:
        _run(case, split, fuse_pool, defect)
    msg = str(e.value)
    assert msg.startswith(where + " (emulated"), msg
    for word in ("frame", "gpu", "ref", "tol"):
        assert word in msg, msg
    if defect == "stale_group":
        assert "frame %d" % (N - 1) in msg, msg


@pytest.mark.parametrize("fuse_pool", [True, False])
def test_split_without_the_lo_pass_is_rejected(case, fuse_pool):
    """Split precision with the x_lo w_hi pass omitted (errors of ~2^-12 of the terms, far inside
    any whole-net tolerance) is beyond the 2^-19 S bound."""
    with pytest.raises(AssertionError) as e:
        _run(case, True, fuse_pool, "no_xlo_pass")
    assert str(e.value).startswith("c3 (emulated<c3>)"), str(e.value)


@pytest.mark.parametrize("fuse_pool", [True, False])
@pytest.mark.parametrize("split", [False, True])
def test_stale_concat_slice_is_rejected(case, split, fuse_pool):
    """A conv's second destination: one 4-channel group of one frame of c3's slice of the concat
    differs from c3's own buffer.  Every per-launch reference passes -- c5 reads the right buffer,
    and the head's reference is fed the concat as it is -- so only the slice check can raise; it
    names the concat, the member, the frame, the element and both values."""
    graph, params, x = case
    net = EmulatedNet(graph, params, x, split, fuse_pool, "stale_concat_slice")
    assert check_concat_slices(EmulatedNet(graph, params, x, split, fuse_pool), graph, [0, N - 1]) == 2
    with pytest.raises(AssertionError) as e:
        check_launches(net, graph, params, x, [0, N - 1], split=split)
    msg = str(e.value)
    assert msg.startswith("cat (concat) member c3 frame %d: " % (N - 1)), msg
    assert "[20, 116)" in msg and "first at (0, 8, " in msg, msg
    for word in ("concat", "member", "tol 0"):
        assert word in msg, msg
    # the defect is in the concat alone, and in the last frame alone
    assert check_concat_slices(net, graph, [0]) == 2
    with pytest.raises(AssertionError):
        check_concat_slices(net, graph, [N - 1])


def test_wrong_net_output_offset_is_rejected(case):
    """The head's slice of net_output is checked as well as its own blob: a head written one channel
    off inside net_output raises."""
    graph, params, x = case
    net = EmulatedNet(graph, params, x, False, True)
    net.blobs["net_output"] = np.roll(net.blobs["net_output"], 1, axis=1)
    with pytest.raises(AssertionError) as e:
        check_launches(net, graph, params, x, [0, N - 1])
    assert "net_output slice" in str(e.value)
