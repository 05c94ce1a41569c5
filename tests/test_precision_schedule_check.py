"""CPU: the mixed-precision per-launch checker (tests/schedule_check.py) accepts a correct net under
a per-layer precision schedule and rejects the two defects the schedule adds to what
tests/test_launch_check.py already injects: a split conv without its x_hi w_lo pass (what a wrong
hi-only kernel would compute) and a non-zero lo left under an fp16 writer.

The stand-in serves blob(), blob_planes() and launch_log() from an emulation of the graph of
tests/test_launch_check.py at 2 x 24 x 40: every blob as its stored (hi, lo) planes, an fp16 conv
reading the hi plane and writing hi only, a split conv reading hi + lo and writing the pair, the
pool selecting the pair of the largest hi + lo.  Convs are evaluated in float64 and rounded at the
stores, so the clean stand-in differs from the references by what a correct kernel may differ by.
"""
import numpy as np
import pytest

from oracle import fp16 as emu
from oracle import split as sp
from tests.launch_check import random_params
from tests.schedule_check import FP16, SPLIT, check_lo_zero, check_schedule
from tests.test_launch_check import H, N, W, graph4

# c3 reads the pool of c2; c4 reads the concat (c5, c3)
SCHEDULES = {
    # c3 hi-only (its source is fp16), c5 fp16 over a split blob, c4 three-product over a concat
    # with an fp16 and a split member
    "fp16_front": dict(c1=FP16, c2=FP16, c3=SPLIT, c5=FP16, c4=SPLIT),
    # split -> fp16 -> split, an fp16 head over the mixed concat
    "alternating": dict(c1=SPLIT, c2=FP16, c3=SPLIT, c5=SPLIT, c4=FP16),
    "split_front": dict(c1=SPLIT, c2=SPLIT, c3=FP16, c5=FP16, c4=FP16),
}


def _pool_planes(hi, lo):
    """2x2 / 2 max pool (even sizes) of (hi, lo) planes: the pair of the largest hi + lo."""
    n, c, h, w = hi.shape
    def windows(a):
        return a.reshape(n, c, h // 2, 2, w // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    s = windows(hi + lo)
    pick = np.argmax(s, axis=4)[..., None]
    return (np.take_along_axis(windows(hi), pick, 4)[..., 0], np.take_along_axis(windows(lo), pick, 4)[..., 0])


class EmulatedMixedNet:
    def __init__(self, graph, params, x, schedule, fuse_pool, defect=None):
        convs, _ = emu.annotate(graph)
        self.planes = {}
        self.log = []
        cur = {"image": (np.asarray(x, np.float32), np.zeros_like(x, np.float32))}
        for l in graph:
            top = l["top"][0]
            if l["type"] == "Convolution":
                c = convs[l["name"]]
                split = schedule[l["name"]] == SPLIT
                w, b, s = [None if a is None else np.array(a, np.float32) for a in params[l["name"]]]
                hi, lo = cur[l["bottom"][0]]
                if split:
                    xin = hi + lo
                    if defect == "no_whi_xlo" and l["name"] == "c3":
                        w = emu.f16(w)     # x_hi w_lo omitted: only w_hi is multiplied
                else:
                    xin, w = emu.f16(hi), emu.f16(w)
                t = sp._act64(sp._conv64(xin, w, b, c["pad"]), c["act"], s).astype(np.float32)
                if l["name"] == "c4":      # the fp32 net output
                    v = (t, np.zeros_like(t))
                else:
                    vh = emu.f16(t)
                    v = (vh, emu.f16(t - vh) if split else np.zeros_like(t))
                if defect == "stale_lo" and l["name"] == "c5":
                    # one lo element of the last frame of c5's slice of the concat buffer (its only
                    # placement; an fp16 writer) left over from an earlier forward
                    v[1][N - 1, 3, 2, 5] = np.float32(2.0 ** -14)
                cur[top] = v
                fused = fuse_pool and l["name"] == "c2"
                if not fused:
                    self.planes[top] = v
                self.log.append((l["name"] + ("+pool" if fused else ""), "emulated<%s>" % l["name"]))
            elif l["type"] == "Pooling":
                cur[top] = self.planes[top] = _pool_planes(*cur[l["bottom"][0]])
                if not fuse_pool:
                    self.log.append(("pool", "emulated_pool"))
            elif l["type"] == "Concat":
                v = tuple(np.concatenate([cur[b][k] for b in l["bottom"]], axis=1) for k in (0, 1))
                cur[top] = self.planes[top] = v

    def launch_log(self):
        return list(self.log)

    def blob_planes(self, name, frames):
        f0, nf = frames
        if name not in self.planes:
            raise RuntimeError(name + ": kept on chip by a fused kernel")
        hi, lo = self.planes[name]
        return hi[f0:f0 + nf].copy(), lo[f0:f0 + nf].copy(), bool(np.any(lo != 0))

    def blob(self, name, frames):
        hi, lo, _ = self.blob_planes(name, frames)
        return hi + lo


@pytest.fixture(scope="module")
def case():
    graph = graph4()
    params = random_params(graph, 71)
    x = np.random.default_rng(72).uniform(-0.5, 0.5, (N, 3, H, W)).astype(np.float32)
    return graph, params, x


def _run(case, schedule, fuse_pool, defect=None):
    graph, params, x = case
    net = EmulatedMixedNet(graph, params, x, schedule, fuse_pool, defect)
    return check_schedule(net, graph, params, x, [0, N - 1], schedule)


@pytest.mark.parametrize("fuse_pool", [True, False])
@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_clean_mixed_emulation_is_accepted(case, name, fuse_pool):
    rows = _run(case, SCHEDULES[name], fuse_pool)
    assert [r.layer for r in rows] == (["c1", "c2+pool", "c3", "c5", "c4"] if fuse_pool
                                       else ["c1", "c2", "c3", "c5", "c4", "p1"])
    assert all(0 <= r.frac < 1 for r in rows)
    # an fp16 unit's float64 sums differ from the reference's fp32 sums: not compared with itself
    assert max(r.frac for r in rows) > 0
    graph, params, x = case
    net = EmulatedMixedNet(graph, params, x, SCHEDULES[name], fuse_pool)
    assert check_lo_zero(net, graph, SCHEDULES[name], [0, N - 1]) > 0


@pytest.mark.parametrize("fuse_pool", [True, False])
def test_split_without_the_wlo_pass_is_rejected(case, fuse_pool):
    """The hi-only conv (c3 after the fp16 front) computing x_hi w_hi alone -- the x_hi w_lo pass
    missing, ~2^-12 of the terms -- is beyond the 2^-19 S bound."""
    with pytest.raises(AssertionError) as e:
        _run(case, SCHEDULES["fp16_front"], fuse_pool, "no_whi_xlo")
    assert str(e.value).startswith("c3 (emulated<c3>)"), str(e.value)


@pytest.mark.parametrize("fuse_pool", [True, False])
def test_stale_lo_under_an_fp16_writer_is_rejected(case, fuse_pool):
    """One non-zero lo element in the fp16 member's slice of a concat whose other member is split:
    every per-launch reference passes (the fp16 unit's hi plane is right, the split head is
    referenced to whatever the concat holds) and the slice equals the member's blob (one memory),
    so only the lo-plane check can raise; it names the blob, the channels, the writer and the frame."""
    graph, params, x = case
    sched = SCHEDULES["fp16_front"]
    with pytest.raises(AssertionError) as e:
        _run(case, sched, fuse_pool, "stale_lo")
    msg = str(e.value)
    assert msg.startswith("c5 (lo plane) channels [0, 20) written by the fp16 conv c5, frame %d" % (N - 1)), msg
    assert "first at (0, 3, 2, 5)" in msg and "tol 0" in msg, msg
    net = EmulatedMixedNet(graph, params, x, sched, fuse_pool, "stale_lo")
    assert check_lo_zero(net, graph, sched, [0]) > 0   # the defect is in the last frame alone
