"""Cases of the PAF score tests: net outputs, hand-written peaks and threshold sets, the oracle's
scores for them, and a plain restatement of getScoreAB's sample count used to prove (on the CPU,
tests/test_paf_cases.py) that the cases contain the lines they claim to.

A case is (geometry, pose model).  Its peaks do not come from NMS: every endpoint is chosen here, so
the clamp outside the map, the degenerate line, the switch points of the sample count n, the count
test at equality and the 63 / 64 / 65 line boundary between the kernels' two lane layouts occur by
construction.  tests/test_gpu_paf_scores.py runs the cases through opk_paf_scores_sources.
"""
import functools

import numpy as np

import oracle
from openpose_amd import synth
from openpose_amd.pose_tables import BODY_25, BODY_135

MAPS_CPU, MAPS_CUDA = 0, 1
MAX_PEAKS = 127
FRAMES = 2
# the bytes a workgroup stages are 8 per source pixel (x and y plane) up to 40 KiB
# name: sources [(h, w)], target (H, W), semantics, scale ratios, staged bytes expected
GEOMETRIES = {
    "G1": dict(sources=[(12, 20)], target=(96, 160), staged=8 * 240),
    "G2": dict(sources=[(12, 20), (9, 15)], target=(96, 160), staged=8 * (240 + 135)),
    "G3a": dict(sources=[(64, 80)], target=(128, 160), staged=40 * 1024),
    "G3b": dict(sources=[(65, 79)], target=(130, 158), staged=0),
    "G4": dict(sources=[(40, 64), (30, 48), (20, 32), (16, 32)], target=(80, 128), staged=0),
    "G5a": dict(sources=[(12, 20)], target=(96, 160), semantics=MAPS_CUDA, staged=0),
    "G5b": dict(sources=[(12, 20), (9, 15)], target=(96, 160), semantics=MAPS_CUDA,
                ratios=(1.0, 0.75), staged=0),
    "G6": dict(sources=[(48, 64)], target=(48, 64), staged=8 * 48 * 64),
}
assert 8 * 64 * 80 == 40 * 1024 and 8 * 65 * 79 > 40 * 1024
assert sum(h * w for h, w in GEOMETRIES["G4"]["sources"]) == 5152

# (inter_th, inter_min_above, nms_th); the first is the product's
DEFAULT_TH = (0.05, 0.95, 0.05)
THRESHOLDS = [DEFAULT_TH, (0.05, 0.5, 0.05), (0.05, 0.0, 0.05), (0.05, 1.0, 0.05),
              (0.05, 1.5, 0.05), (0.05, -0.1, 0.05), (0.0, 0.95, 0.05), (-0.2, 0.5, 0.05),
              (0.05, 0.9, 0.3)]

# BODY_25 peak counts per part, frame 0: the pairs' line counts nA * nB hold 0 with either side
# empty, 1, 9 (1 x 9 and 3 x 3), 63, 64, 65, 127 (1 x 127) and 127 x 127 twice
COUNTS_25 = [7, 8, 8, 3, 21, 2, 4, 16, 1, 127, 127, 127, 1, 13, 5, 9, 3, 1, 3, 0, 4, 3, 0, 5, 0]
# the designed line counts and a pair of frame 0 that has each
LINE_COUNTS = {0: (11, 22), 1: (8, 12), 9: (16, 18), 63: (0, 15), 64: (1, 2), 65: (13, 14),
               127: (8, 9), 127 * 127: (9, 10)}
# the G6 lines: pair (1, 2), line i joins peak i of part 1 to peak i of part 2 along row G6_ROWS[i]
G6_PAIR = 1
G6_ROWS = [3 + 5 * i for i in range(8)]
G6_SPANS = [80.0] * 4 + [124.0] * 4           # n = 20 and n = 25
G6_FAILS = [0, 1, 2, 3, 0, 1, 2, 3]           # samples set below inter_th
# which samples fail: early ones (the line can leave its loop at once) and late ones
G6_FAIL_AT = [[], [9], [0, 1], [2, 7, 11], [], [12], [3, 10], [0, 1, 2]]


def table(model=BODY_25):
    return oracle.pose_tables()[model]


def channels(t):
    return t["parts"] + int(t["bkg"]) + len(t["map_idx"])


def pair_parts(t, q):
    return t["pairs"][2 * q], t["pairs"][2 * q + 1]


def pair_planes(t, q):
    base = t["parts"] + int(t["bkg"])
    return base + t["map_idx"][2 * q], base + t["map_idx"][2 * q + 1]


def _g6_pixels(i):
    """x of the distinct pixels the samples of G6 line i read (the clamped tail shares W - 1)."""
    n = 20 if G6_SPANS[i] == 80.0 else 25
    step = np.float32(G6_SPANS[i]) / np.float32(n)
    return [int(np.float32(s) * step + np.float32(0.5)) for s in range(n)]


@functools.lru_cache(maxsize=None)
def sources(name, model=BODY_25):
    """The net outputs of a geometry: a list of [FRAMES, C, h, w] float32 arrays."""
    g = GEOMETRIES[name]
    t = table(model)
    C, base = channels(t), t["parts"] + int(t["bkg"])
    rng = np.random.default_rng(sum(map(ord, name)) + 1000 * model)
    out = []
    if name == "G6":   # a uniform PAF field of (1, 0); chosen pixels of the G6 rows below inter_th
        f = np.zeros((FRAMES, C, 48, 64), np.float32)
        f[:, base::2] = 1.0
        px = pair_planes(t, G6_PAIR)[0]
        for i, row in enumerate(G6_ROWS):
            xs = _g6_pixels(i)
            for s in G6_FAIL_AT[i]:
                assert xs[s] < 63 and xs.count(xs[s]) == 1
                f[:, px, row, xs[s]] = -1.0
        return [f]
    # smooth waves in [-1, 1] on normalised coordinates (the scales of a case then agree on where
    # lines pass) plus a few synthetic people
    k = rng.uniform(-1.5, 1.5, (FRAMES, C, 2))
    ph = rng.uniform(0, 2 * np.pi, (FRAMES, C))
    for si, (h, w) in enumerate(g["sources"]):
        v, u = np.mgrid[0:h, 0:w]
        arg = (k[..., 0, None, None] * (u / w) + k[..., 1, None, None] * (v / h)) * 2 * np.pi
        f = np.sin(arg + ph[..., None, None]).astype(np.float32)
        for b in range(FRAMES):
            f[b] += synth.overlay(3, h, w, seed=500 + 10 * si + b, table=t)
        out.append(np.ascontiguousarray(f, np.float32))
    return out


def _points(rng, n, H, W):
    """n endpoints inside the map with fractional coordinates"""
    return np.stack([rng.uniform(0.3, W - 1.3, n), rng.uniform(0.3, H - 1.3, n)], 1)


@functools.lru_cache(maxsize=None)
def peaks(name, model=BODY_25):
    """[FRAMES, parts, MAX_PEAKS + 1, 3] float32: the count in [p, 0, 0], then (x, y, score)."""
    H, W = GEOMETRIES[name]["target"]
    t = table(model)
    P = t["parts"]
    rng = np.random.default_rng(77 + sum(map(ord, name)) + 1000 * model)
    out = np.zeros((FRAMES, P, MAX_PEAKS + 1, 3), np.float32)
    for b in range(FRAMES):
        if model == BODY_25 and b == 0:
            counts = list(COUNTS_25)
        else:   # other totals than frame 0; one pair with more than 64 lines
            counts = [int(c) for c in rng.integers(0, 9, P)]
            a0, b0 = pair_parts(t, 0)
            counts[a0], counts[b0] = 9, 11
        for p in range(P):
            out[b, p, 0, 0] = counts[p]
            out[b, p, 1:counts[p] + 1, :2] = _points(rng, counts[p], H, W)
            out[b, p, 1:counts[p] + 1, 2] = rng.uniform(0.1, 1.0, counts[p])
        if model != BODY_25 or b != 0:
            continue
        xy = out[b, :, 1:, :2]   # [part, peak] -> (x, y)
        # pair (12, 13), 1 x 13 lines from P: 300 wide (n capped at 25), coincident, and ends
        # outside the map on each side
        Pt = np.float32([3.5, 2.25])
        xy[12, 0] = Pt
        xy[13, 0] = Pt + np.float32([300, 10])
        xy[13, 1] = Pt
        xy[13, 2] = [-0.75, 5.5]
        xy[13, 3] = [W - 1 + 0.6, 7.25]
        xy[13, 4] = [20.5, H + 3]
        # pair (13, 14), from A (= peak 5 of part 13): max(|dx|, |dy|) at the switch points of n
        A = np.float32([10.25, 20.5])
        xy[13, 5] = A
        xy[14, 0] = A + np.float32([4.9, 0])
        xy[14, 1] = A + np.float32([0.5, 6.0])
        xy[14, 2] = A + np.float32([6.1, 1])
        xy[14, 3] = A + np.float32([120.0, 3])
        xy[14, 4] = A + np.float32([-2, 120.1])
        # pair (16, 18) at the origin: 5e-7 apart (norm <= 1e-6: 0) and 2e-6 apart
        xy[16, 0] = [0, 0]
        xy[18, 0] = [5e-7, 0]
        xy[18, 1] = [0, 2e-6]
        # pair (3, 4): ends within 0.3 .. 0.75 px of peak 0 of part 3, in every direction (lines
        # shorter than sqrt(W * H) / 150 that pass and that fail)
        ang = np.arange(12) * (2 * np.pi / 12) + 0.1
        r = 0.3 + 0.45 * (np.arange(12) % 3) / 2
        xy[4, :12] = xy[3, 0] + np.stack([r * np.cos(ang), r * np.sin(ang)], 1).astype(np.float32)
        if name == "G6":
            for i, row in enumerate(G6_ROWS):
                xy[1, i] = [0, row]
                xy[2, i] = [G6_SPANS[i], row]
    return out


def counts_of(pk, t, q):
    a, b = pair_parts(t, q)
    return int(pk[a, 0, 0] + np.float32(0.5)), int(pk[b, 0, 0] + np.float32(0.5))


def total_lines(pk, t):
    return sum(int(np.prod(counts_of(pk, t, q))) for q in range(len(t["pairs"]) // 2))


@functools.lru_cache(maxsize=None)
def heat(name, model=BODY_25):
    """The oracle's merged map of each frame: [FRAMES][C, H, W]."""
    g = GEOMETRIES[name]
    H, W = g["target"]
    src = sources(name, model)
    if g.get("semantics", MAPS_CPU) == MAPS_CUDA:
        maps = [oracle.resize_merge_cuda([s[b] for s in src], H, W, g.get("ratios"))
                for b in range(FRAMES)]
        assert all(m is not None for m in maps)
        return maps
    return [oracle.resize_merge([s[b] for s in src], H, W) for b in range(FRAMES)]


@functools.lru_cache(maxsize=None)
def reference(name, model=BODY_25, th=DEFAULT_TH):
    """The oracle's dense score table of each frame: [FRAMES][npairs, MAX_PEAKS, MAX_PEAKS]."""
    pk, t = peaks(name, model), table(model)
    return [oracle.pair_scores_table(heat(name, model)[b], pk[b], t, inter_th=th[0],
                                     inter_min_above=th[1], nms_th=th[2]) for b in range(FRAMES)]


def compact(ref, pk, t):
    """The compact record body of one frame: the nA x nB blocks of the pairs in order, row-major."""
    out = []
    for q in range(len(t["pairs"]) // 2):
        na, nb = counts_of(pk, t, q)
        out.append(ref[q, :na, :nb].ravel())
    return np.concatenate(out) if out else np.zeros(0, np.float32)


# ---- getScoreAB's sample count, restated plainly (float32 throughout, one operation at a time) ---
def samples_needed(n, inter_min_above):
    """the fewest passing samples c of n with float(c) / float(n) > inter_min_above (n + 1: none)"""
    for c in range(n + 1):
        if np.float32(c) / np.float32(n) > np.float32(inter_min_above):
            return c
    return n + 1


def line_facts(hm, pk, t, q, th=DEFAULT_TH):
    """Every line of pair q of one frame (row-major i, j) as arrays: vmax, n, norm, ends a and b,
    passed [lines, 25] (sample s above inter_th; False past n), count, and the restated score."""
    f32 = np.float32
    pa, pb = pair_parts(t, q)
    na, nb = counts_of(pk, t, q)
    H, W = hm.shape[1:]
    a = np.repeat(pk[pa, 1:na + 1, :2], nb, 0).astype(f32)
    b = np.tile(pk[pb, 1:nb + 1, :2], (na, 1)).astype(f32)
    mx, my = (hm[c] for c in pair_planes(t, q))
    vx, vy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
    vmax = np.maximum(np.abs(vx), np.abs(vy))
    n = np.clip((np.sqrt(f32(5) * vmax) + f32(0.5)).astype(np.int64), 5, 25)
    norm = np.sqrt(vx * vx + vy * vy)
    live = norm.astype(np.float64) > 1e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        ux, uy = vx / norm, vy / norm
        sx, sy = vx / n.astype(f32), vy / n.astype(f32)
    passed = np.zeros((len(a), 25), bool)
    total = np.zeros(len(a), f32)
    for s in range(25):
        x = np.clip((a[:, 0] + f32(s) * sx + f32(0.5)).astype(np.int64), 0, W - 1)
        y = np.clip((a[:, 1] + f32(s) * sy + f32(0.5)).astype(np.int64), 0, H - 1)
        x, y = np.where(live, x, 0), np.where(live, y, 0)
        v = ux * mx[y, x] + uy * my[y, x]
        ok = live & (s < n) & (v > f32(th[0]))
        passed[:, s] = ok
        total = total + np.where(ok, v, f32(0))
    count = passed.sum(1)
    near = norm.astype(np.float64) < np.sqrt(float(W * H)) / 150
    with np.errstate(divide="ignore", invalid="ignore"):
        wins = live & (count.astype(f32) / n.astype(f32) > f32(th[1]))
        score = np.where(wins, total / count.astype(f32),
                         np.where(live & near, f32(np.float64(f32(th[2])) + 1e-6), f32(0)))
    return dict(a=a, b=b, vmax=vmax, n=n, norm=norm, live=live, passed=passed, count=count,
                wins=wins, near=near, score=score.astype(f32))


def break_sample(passed, n, needed):
    """the sample at which a line leaves the loop under the early-exit rule (more than n - needed
    samples failed), or None when it runs to its end"""
    fails = 0
    for s in range(n):
        if not passed[s]:
            fails += 1
            if fails > n - needed:
                return s
    return None
