"""The PAF score cases (tests/paf_cases.py) contain what they claim: proved with the oracle alone.

The GPU test compares every score of these cases with the oracle; that comparison is only worth as
much as the lines it covers.  Here each class of line the cases were built for is shown to be
present among the compared lines, from the oracle's merged map and a plain restatement of
getScoreAB's sample count -- which is itself held to the oracle's scores, bit for bit.
"""
import numpy as np
import pytest

from tests import paf_cases as pc

f32 = np.float32


def _facts(name, frame=0, th=pc.DEFAULT_TH, model=pc.BODY_25):
    """line_facts of every pair of one frame, with the oracle's scores of the same lines"""
    t = pc.table(model)
    hm, pk = pc.heat(name, model)[frame], pc.peaks(name, model)[frame]
    ref = pc.reference(name, model, th)[frame]
    out = []
    for q in range(len(t["pairs"]) // 2):
        na, nb = pc.counts_of(pk, t, q)
        if na * nb == 0:
            continue
        f = pc.line_facts(hm, pk, t, q, th)
        f["ref"] = ref[q, :na, :nb].ravel()
        f["q"] = q
        out.append(f)
    return out


def _all(facts, key):
    return np.concatenate([f[key] for f in facts])


@pytest.mark.parametrize("name", sorted(pc.GEOMETRIES))
def test_restated_scores_are_the_oracles(name):
    """The restatement gives the oracle's score for every line of every frame (NaN where a line
    passes the count test with no sample, both), so its sample counts are the oracle's."""
    for th in (pc.THRESHOLDS if name in ("G1", "G6") else [pc.DEFAULT_TH]):
        for b in range(pc.FRAMES):
            for f in _facts(name, b, th):
                np.testing.assert_array_equal(f["score"], f["ref"], err_msg="%s pair %d" % (name, f["q"]))


def test_line_counts():
    """Frame 0 has pairs with 0 lines (either side empty), 1, 9, 63, 64, 65, 127 and 127 x 127
    (twice); the last half-wave of a 9-line pair holds one line; the frames' totals differ."""
    t = pc.table()
    pk = pc.peaks("G1")
    by_parts = {pc.pair_parts(t, q): pc.counts_of(pk[0], t, q) for q in range(26)}
    for lines, parts in pc.LINE_COUNTS.items():
        assert int(np.prod(by_parts[parts])) == lines, (lines, parts)
    assert by_parts[(11, 22)][0] > 0 and by_parts[(11, 22)][1] == 0     # B empty
    assert by_parts[(22, 23)][0] == 0 and by_parts[(22, 23)][1] > 0     # A empty
    assert by_parts[(8, 9)] == (1, 127) and by_parts[(16, 18)] == (3, 3)
    assert by_parts[(9, 10)] == by_parts[(10, 11)] == (127, 127)
    assert sum(1 for c in by_parts.values() if c[0] * c[1] > 256) == 2   # more lines than lanes
    for name in pc.GEOMETRIES:
        p = pc.peaks(name)
        assert np.array_equal(p[0, :, 0, 0], pk[0, :, 0, 0])
        assert pc.total_lines(p[0], t) != pc.total_lines(p[1], t)
        assert max(np.prod(pc.counts_of(p[1], t, q)) for q in range(26)) >= 64
    t135 = pc.table(pc.BODY_135)
    p = pc.peaks("G1", pc.BODY_135)
    assert pc.total_lines(p[0], t135) != pc.total_lines(p[1], t135)
    assert all(max(np.prod(pc.counts_of(p[b], t135, q)) for q in range(len(t135["pairs"]) // 2)) >= 64
               for b in range(2))


@pytest.mark.parametrize("name", ["G1", "G3b", "G4", "G5b"])
def test_endpoint_classes(name):
    H, W = pc.GEOMETRIES[name]["target"]
    facts = _facts(name)
    a, b = _all(facts, "a"), _all(facts, "b")
    vmax, n, norm = _all(facts, "vmax"), _all(facts, "n"), _all(facts, "norm")
    live, wins, near, ref = (_all(facts, k) for k in ("live", "wins", "near", "ref"))
    inside = lambda p: (p[:, 0] > 0) & (p[:, 0] < W - 1) & (p[:, 1] > 0) & (p[:, 1] < H - 1)
    frac = lambda p: (p[:, 0] != np.floor(p[:, 0])) & (p[:, 1] != np.floor(p[:, 1]))
    assert (inside(a) & inside(b) & frac(a) & frac(b)).sum() > 100
    # ends outside the map on each side
    assert (b[:, 0] == f32(-0.75)).any() and (b[:, 0] == f32(W - 1 + 0.6)).any()
    assert (b[:, 1] == f32(H + 3)).any() and (b[:, 0] > W + 100).any()
    # the degenerate lines: coincident ends, and 5e-7 apart at the origin; 2e-6 apart is a line
    coincide = (vmax == 0)
    assert coincide.any() and (ref[coincide] == 0).all()
    tiny = (norm > 0) & ~live
    assert tiny.any() and (ref[tiny] == 0).all() and np.allclose(norm[tiny], 5e-7, rtol=1e-3)
    assert (live & (norm < 3e-6)).any()
    # the switch points of n
    for v, want in ((4.9, 5), (6.0, 5), (6.1, 6), (120.0, 24), (120.1, 25), (300.0, 25)):
        hit = np.abs(vmax - f32(v)) < 1e-4
        assert hit.any() and (n[hit] == want).all(), (v, want, n[hit])
    # failing lines shorter and longer than sqrt(W * H) / 150, and passing ones of both kinds
    reject = f32(np.float64(f32(0.05)) + 1e-6)
    assert (live & ~wins & near).any() and (ref[live & ~wins & near] == reject).all()
    assert (live & ~wins & ~near).sum() > 100 and (ref[live & ~wins & ~near] == 0).all()
    assert (wins & near).any() and (wins & ~near).any()


def test_thresholds_change_the_outcome():
    """On G1 every threshold set gives another split of the lines: none pass at 1.0 and 1.5, every
    line passes at -0.1 (some without a sample: 0 / 0), and the fallback follows nms_th."""
    wins = {}
    for th in pc.THRESHOLDS:
        facts = _facts("G1", 0, th)
        wins[th] = _all(facts, "wins")
        live = _all(facts, "live")
        if th[1] >= 1.0:
            assert not wins[th].any()
        if th[1] < 0:
            assert wins[th][live].all() and np.isnan(_all(facts, "ref")).any()
    base = wins[pc.DEFAULT_TH].sum()
    assert 0 < base < wins[(0.05, 0.5, 0.05)].sum() < wins[(0.05, 0.0, 0.05)].sum()
    assert wins[(0.0, 0.95, 0.05)].sum() > base
    th = pc.THRESHOLDS[-1]
    assert th[2] != th[0]
    facts = _facts("G1", 0, th)
    short_fail = _all(facts, "live") & ~_all(facts, "wins") & _all(facts, "near")
    assert short_fail.any()
    assert (_all(facts, "ref")[short_fail] == f32(np.float64(f32(th[2])) + 1e-6)).all()


@pytest.mark.parametrize("th", [pc.DEFAULT_TH, pc.THRESHOLDS[-1]])
def test_g6_exact_pass_counts(th):
    """The G6 lines have exactly k passing samples for every k from n - 3 to n, for n = 20 and
    n = 25: lines with exactly `needed` and `needed - 1` passing samples exist for both n --
    19 / 20 against 0.95f is equality and fails; they sit in a 64-line pair."""
    t = pc.table()
    assert pc.samples_needed(20, 0.95) == 20 and pc.samples_needed(25, 0.95) == 24
    assert pc.samples_needed(20, 0.9) == 19 and pc.samples_needed(25, 0.9) == 23
    assert pc.samples_needed(5, 1.0) == 6 and pc.samples_needed(5, -0.1) == 0
    pk = pc.peaks("G6")[0]
    assert pc.counts_of(pk, t, pc.G6_PAIR) == (8, 8)
    f = pc.line_facts(pc.heat("G6")[0], pk, t, pc.G6_PAIR, th)
    ref = pc.reference("G6", pc.BODY_25, th)[0][pc.G6_PAIR, :8, :8].ravel()
    seen = set()
    for i in range(8):
        l = 9 * i   # line i -> i
        n = int(f["n"][l])
        assert n == (20 if i < 4 else 25)
        assert int(f["count"][l]) == n - pc.G6_FAILS[i]
        need = pc.samples_needed(n, th[1])
        assert bool(f["wins"][l]) == (int(f["count"][l]) >= need)
        assert (ref[l] == 1.0) == bool(f["wins"][l]) and ref[l] in (0.0, 1.0)
        seen.add((n, int(f["count"][l]) - need))
    for n in (20, 25):
        assert (n, 0) in seen and (n, -1) in seen


def test_early_exit_lines():
    """Among the compared lines are failing ones that leave the sample loop before their last
    sample (at the first sample, in the middle and at the last but one), failing ones that run to
    the end, and passing ones with a failing sample."""
    breaks, full, dented = set(), 0, 0
    for name in ("G1", "G6"):
        for f in _facts(name):
            for l in range(len(f["n"])):
                if not f["live"][l]:
                    continue
                n = int(f["n"][l])
                need = pc.samples_needed(n, pc.DEFAULT_TH[1])
                s = pc.break_sample(f["passed"][l], n, need)
                assert (s is None) == bool(f["wins"][l])   # the rule breaks exactly the losers
                if s is not None:
                    breaks.add("first" if s == 0 else "last" if s == n - 1 else "middle")
                dented += bool(f["wins"][l]) and int(f["count"][l]) < n
    assert breaks == {"first", "middle", "last"}, breaks
    assert dented > 0
    # with inter_min_above 0.5 a loser can run to its last sample
    for f in _facts("G1", 0, (0.05, 0.5, 0.05)):
        for l in np.flatnonzero(f["live"] & ~f["wins"]):
            n = int(f["n"][l])
            s = pc.break_sample(f["passed"][l], n, pc.samples_needed(n, 0.5))
            full += s == n - 1
    assert full > 0
