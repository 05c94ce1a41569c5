"""Keypoint-render inputs that tests/test_render.py's people_on() never produces: people off the
frame (the box that is not grown when a coordinate maximum stays 0), crowds that straddle the frame
edge, coordinates far from every tile, zero-length and axis-parallel limbs, non-finite coordinates
and scores, scores on the threshold, more than 256 hands / faces (the second round of the people
compaction in kernels/render.hip) and frames smaller than one 32x8 tile.

Plain numpy, seeded.  case(name) returns (frame size (w, h), layer kind, keypoints float32
[people, parts, 3], options); oracle_render(name) is the CPU oracle's drawing of it on frame_of(name),
computed once per process and shared (callers must not write into what it returns).

tests/test_render_edge_cases.py holds each case to what it claims, by the oracle alone;
tests/test_gpu_render_edges.py holds the kernels to the oracle on them."""
import functools

import numpy as np

import oracle
from openpose_amd.api import _LAYER_THRESHOLD, LAYER_FACE, LAYER_HAND, LAYER_POSE
from tests.test_gpu_output_frames import ORACLE, PARTS

# RenderLayer's default render thresholds, which tests/test_gpu_output_frames.py draws with
THRESHOLD = _LAYER_THRESHOLD
ALPHA = 0.6
CROWD_SIZE = (320, 96)     # hands* / faces*
TINY = {"tiny-1x1": (1, 1), "tiny-5x3": (5, 3), "tiny-31x7": (31, 7), "tiny-32x8": (32, 8)}

POSE_CASES = ["left", "top", "touch0", "straddle", "far", "coincident-on", "coincident-off", "axis",
              "nonfinite", "ties-at", "ties-above"] + sorted(TINY)
CROWD_CASES = ["hands300", "faces300", "hands256", "hands257", "hands1024"]
CASES = POSE_CASES + CROWD_CASES
# cases whose oracle render marks no pixel ambiguous: the kernels must match on every pixel
EXACT = ["left", "top", "touch0", "coincident-on", "coincident-off", "nonfinite", "ties-at",
         "ties-above"] + sorted(TINY)
# the part of `left` / `touch0` (`top`) that sits 1.0 outside column (row) 0
OUTSIDE_PART, OUTSIDE_AT = 4, 200.0
TOUCH_PART, TOUCH_AT = 7, 300.5


def _off_edge(axis, seed, touch=False):
    """One BODY_25 person on 640x480 with every coordinate of `axis` (0: x, 1: y) in [-30, -0.5]:
    that coordinate's maximum stays exactly 0 and the box is not grown.  The other axis spans 440
    (left) / 600 (top) pixels, so the person's scale clamps to 1."""
    w, h = 640, 480
    rng = np.random.default_rng(seed)
    kp = np.zeros((1, 25, 3), np.float32)
    along = (h, w)[axis]
    kp[0, :, axis] = rng.uniform(-30.0, -0.5, 25)
    kp[0, :, 1 - axis] = rng.uniform(20.0, along - 20.0, 25)
    kp[0, 0, 1 - axis], kp[0, 1, 1 - axis] = 20.0, along - 20.0
    kp[0, :, 2] = rng.uniform(0.2, 1.0, 25)
    kp[0, OUTSIDE_PART, axis], kp[0, OUTSIDE_PART, 1 - axis] = -1.0, OUTSIDE_AT
    if touch:
        kp[0, TOUCH_PART, axis], kp[0, TOUCH_PART, 1 - axis] = 0.0, TOUCH_AT
    return (w, h), LAYER_POSE, kp, {}


def _people(w, h, n, parts, seed, spread=0.15, lo=0.1, hi=0.9):
    """people_on() of tests/test_render.py with the centres uniform in [lo, hi] of the frame.  That
    function stays as it is (the existing render tests draw from it), so this one restates it;
    tests/test_render_edge_cases.py holds the two together at people_on's [0.1, 0.9]."""
    rng = np.random.default_rng(seed)
    kp = np.zeros((n, parts, 3), np.float32)
    for p in range(n):
        cx, cy = rng.uniform(lo, hi) * w, rng.uniform(lo, hi) * h
        r = spread * min(w, h) * rng.uniform(0.5, 1.5)
        kp[p, :, 0] = cx + rng.uniform(-r, r, parts)
        kp[p, :, 1] = cy + rng.uniform(-r, r, parts)
        kp[p, :, 2] = rng.uniform(0, 1, parts)
    kp[..., 2][kp[..., 2] < 0.15] = 0.0
    return kp


def _straddle(seed=6):
    w, h = 320, 240
    return (w, h), LAYER_POSE, _people(w, h, 40, 25, seed, lo=-0.2, hi=1.2), {"googly": True}


def _nonfinite(seed=2):
    size, kind, kp, opts = _straddle()
    rng = np.random.default_rng(seed)
    drawn = np.argwhere(kp[..., 2] > THRESHOLD[kind])
    picks = drawn[rng.choice(len(drawn), 17, replace=False)]
    bad = [np.nan, np.inf, -np.inf]
    for i, (p, part) in enumerate(picks[:12]):
        kp[p, part, i % 2] = bad[(i // 2) % 3]     # each value in an x and in a y, twice
    for p, part in picks[12:]:
        kp[p, part, 2] = np.nan
    return size, kind, kp, opts


def _far():
    """Three people around +-1e6 and one around 1e4, each person's parts within 100 of its centre:
    boxes (one of them reaches column 0, one pixel (0, 0)) and limbs far from every tile."""
    rng = np.random.default_rng(9)
    centres = [(1e6, 1e6), (-1e6, -1e6), (-1e6, 120.0), (1e4, -1e4)]
    kp = np.zeros((4, 25, 3), np.float32)
    for p, (cx, cy) in enumerate(centres):
        kp[p, :, 0] = cx + rng.uniform(-100, 100, 25)
        kp[p, :, 1] = cy + rng.uniform(-100, 100, 25)
        kp[p, :, 2] = rng.uniform(0.2, 1.0, 25)
    return (320, 240), LAYER_POSE, kp, {}


def _coincident(x, y):
    kp = np.zeros((1, 25, 3), np.float32)
    kp[0, :, 0], kp[0, :, 1], kp[0, :, 2] = x, y, 0.9
    return (320, 240), LAYER_POSE, kp, {}


def _tree(pairs):
    """(parent, child) in an order that visits every parent first, from part 1."""
    pairs = [(pairs[2 * i], pairs[2 * i + 1]) for i in range(len(pairs) // 2)]
    seen, order = {1}, []
    while len(order) < len(pairs):
        for a, b in pairs:
            if a in seen and b not in seen:
                order.append((a, b))
                seen.add(b)
            elif b in seen and a not in seen:
                order.append((b, a))
                seen.add(a)
    return order


def _axis(seed=2):
    """Three BODY_25 skeletons whose limbs are all exactly horizontal or vertical, between integer
    coordinates (angles 0, pi, +-pi/2: the arguments where sinf / cosf return their smallest
    values)."""
    w, h = 320, 240
    rng = np.random.default_rng(seed)
    order = _tree(oracle.render_tables()["BODY_25"]["pairs"])
    kp = np.zeros((3, 25, 3), np.float32)
    for p in range(3):
        kp[p, 1, :2] = rng.integers(60, w - 60), rng.integers(60, h - 60)
        for a, b in order:
            step = int(rng.integers(6, 41)) * int(rng.choice([-1, 1]))
            kp[p, b, :2] = kp[p, a, :2]
            kp[p, b, int(rng.integers(0, 2))] += step
        kp[p, :, 2] = 0.9
    return (w, h), LAYER_POSE, kp, {}


def _ties(above):
    w, h = 320, 240
    kp = _people(w, h, 6, 25, seed=4)
    th = np.float32(THRESHOLD[LAYER_POSE])
    kp[..., 2] = np.nextafter(th, np.float32(1)) if above else th
    return (w, h), LAYER_POSE, kp, {}


def crowd(kind, n, seed, above):
    """n hands (faces) with centres uniform over CROWD_SIZE and parts within +-12 px; `above` of each
    one's parts score above the threshold."""
    w, h = CROWD_SIZE
    parts, th = PARTS[kind], THRESHOLD[kind]
    rng = np.random.default_rng(seed)
    kp = np.zeros((n, parts, 3), np.float32)
    cx, cy = rng.uniform(0, w, (n, 1)), rng.uniform(0, h, (n, 1))
    kp[..., 0] = cx + rng.uniform(-12, 12, (n, parts))
    kp[..., 1] = cy + rng.uniform(-12, 12, (n, parts))
    kp[..., 2] = rng.uniform(0, 0.9 * th, (n, parts))
    for p in range(n):
        kp[p, rng.choice(parts, above, replace=False), 2] = rng.uniform(th + 0.05, 1.0, above)
    return (w, h), kind, kp, {}


def _tiny(name, seed=0):
    """Two people with parts in [-3, w + 3] x [-3, h + 3].  The first has every part drawn at
    fractional coordinates (limbs); the second sits on integer coordinates with only parts that no
    limb joins above the threshold (circles on pixel centres without a limb ending on one, which
    would be an ambiguous pixel), one of them on the frame's first and one on its last pixel."""
    w, h = TINY[name]
    rng = np.random.default_rng(seed + 31 * w + h)
    kp = np.zeros((2, 25, 3), np.float32)
    kp[..., 0] = rng.uniform(-3, w + 3, (2, 25))
    kp[..., 1] = rng.uniform(-3, h + 3, (2, 25))
    kp[0, :, 2] = rng.uniform(0.2, 1.0, 25)
    kp[1, :, :2] = np.clip(np.rint(kp[1, :, :2]), -3, (w + 3, h + 3))
    lone = [part for part, d in sorted(_depths().items()) if d % 2 == 0]   # no two share a limb
    kp[1, lone, 2] = 0.8
    kp[1, lone[0], :2] = 0, 0
    kp[1, lone[1], :2] = w - 1, h - 1
    return (w, h), LAYER_POSE, kp, {}


@functools.lru_cache(None)
def _depths():
    """Each BODY_25 part's distance from part 1 along the limbs (a tree)."""
    d = {1: 0}
    for a, b in _tree(oracle.render_tables()["BODY_25"]["pairs"]):
        d[b] = d[a] + 1
    return d


_BUILDERS = {
    "left": lambda: _off_edge(0, 1),
    "top": lambda: _off_edge(1, 2),
    "touch0": lambda: _off_edge(0, 3, touch=True),
    "straddle": _straddle,
    "far": _far,
    "coincident-on": lambda: _coincident(160.0, 120.0),
    "coincident-off": lambda: _coincident(160.5, 120.25),
    "axis": _axis,
    "nonfinite": _nonfinite,
    "ties-at": lambda: _ties(False),
    "ties-above": lambda: _ties(True),
    "hands300": lambda: crowd(LAYER_HAND, 300, 41, 5),
    "faces300": lambda: crowd(LAYER_FACE, 300, 42, 6),
    "hands256": lambda: crowd(LAYER_HAND, 256, 40, 5),
    "hands257": lambda: crowd(LAYER_HAND, 257, 40, 5),
    "hands1024": lambda: crowd(LAYER_HAND, 1024, 42, 3),
}
for _name in TINY:
    _BUILDERS[_name] = functools.partial(_tiny, _name)


def case(name):
    """(frame size (w, h), kind, keypoints [people, parts, 3], options); a fresh copy each call."""
    return _BUILDERS[name]()


def oracle_kwargs(kind, opts):
    """oracle.render_keypoints' arguments of a layer kind."""
    return dict(parts=PARTS[kind], threshold=THRESHOLD[kind], alpha=ALPHA,
                eyes=(15, 16) if opts.get("googly") else (-1, -1), **ORACLE[kind])


def frame_of(name):
    (w, h), _, _, _ = case(name)
    return np.random.default_rng(len(name) + w).uniform(0, 255, (h, w, 3)).astype(np.float32)


@functools.lru_cache(None)
def oracle_render(name, blend=True):
    """(drawn frame, ambiguous mask) of the case on frame_of(name); shared: do not write into it."""
    _, kind, kp, opts = case(name)
    out, amb = oracle.render_keypoints(frame_of(name), kp, blend=blend, **oracle_kwargs(kind, opts))
    out.setflags(write=False)
    amb.setflags(write=False)
    return out, amb
