"""Person ids across frames as include/opk.h defines them ("Person ids across frames"), restated in
numpy fp32 from that text alone: grey image, Gaussian pyramid, one pyramidal Lucas-Kanade point,
the greedy matcher and the tracker's bookkeeping -- plus the cases the CPU and GPU tests share.

Every float operation below is a numpy float32 operation (one rounding each); the five sums of a
level are np.add.accumulate rows, which add strictly left to right."""
import numpy as np

F = np.float32
LK_POINT = np.dtype([("frame_i", "<i4"), ("frame_j", "<i4"), ("x", "<f4"), ("y", "<f4"),
                     ("status", "<i4")])
CONFIDENCE, INLIER_RATIO, DISTANCE, FRAMES_TO_DELETE = 0.1, 0.5, 30.0, 10


# ---- grey + pyramid ---------------------------------------------------------------------------
def grey(bgr):
    """uint8 [..., 3] BGR -> float32 [...]: (1868 B + 9617 G + 4899 R + 8192) >> 14."""
    c = np.asarray(bgr).astype(np.int64)
    return ((1868 * c[..., 0] + 9617 * c[..., 1] + 4899 * c[..., 2] + 8192) >> 14).astype(F)


def reflect(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


_TAPS = (1, 4, 6, 4, 1)


def _taps_along(img, axis, reverse):
    """Sum of the five taps along `axis` around the even samples, in float32, one add at a time."""
    n = img.shape[axis]
    out_n = (n + 1) // 2
    acc = None
    for k in (range(4, -1, -1) if reverse else range(5)):
        idx = [reflect(2 * o + k - 2, n) for o in range(out_n)]
        term = F(_TAPS[k]) * np.take(img, idx, axis=axis)
        acc = term if acc is None else acc + term
    return acc.astype(F)


def pyr_down(img, order=0):
    """The next level of a float32 level.  order 0: taps in x, then in y, each left to right, as
    the definition words it; order 1: y first, taps right to left -- the definition says the
    result is exact, so both must agree bit for bit."""
    img = np.asarray(img, F)
    if order == 0:
        s = _taps_along(_taps_along(img, 1, False), 0, False)
    else:
        s = _taps_along(_taps_along(img, 0, True), 1, True)
    return (s * F(1.0 / 256.0)).astype(F)


def pyramid(g, levels=3, order=0):
    """[level 0, ...] of a grey image."""
    out = [np.asarray(g, F)]
    for _ in range(levels - 1):
        out.append(pyr_down(out[-1], order))
    return out


# ---- Lucas-Kanade -----------------------------------------------------------------------------
def _trunc(v):
    with np.errstate(invalid="ignore"):
        inside = np.abs(v) < F(2.0 ** 30)
        t = np.trunc(np.where(inside, v, F(0))).astype(np.int64)
    return np.where(inside, t, -(1 << 30))


def _seq_sum(prod):
    """Row sums of float32 [points, 441], accumulated left to right from +0."""
    z = np.zeros((prod.shape[0], 1), F)
    return np.add.accumulate(np.concatenate([z, prod.astype(F)], axis=1), axis=1, dtype=F)[:, -1]


_DI, _DJ = [a.reshape(-1) for a in np.meshgrid(np.arange(-10, 11), np.arange(-10, 11), indexing="ij")]


def _lk_pair(pyr_i, pyr_j, x, y):
    """Points (float32 arrays, status 0, coordinates in range) from pyramid I to pyramid J."""
    n = x.shape[0]
    pix, piy = x * F(0.25), y * F(0.25)
    pjx, pjy = pix.copy(), piy.copy()
    status = np.zeros(n, np.int32)
    for lv in (2, 1, 0):
        I, J = pyr_i[lv], pyr_j[lv]
        h, w = I.shape
        xi, yi, xj, yj = _trunc(pix), _trunc(piy), _trunc(pjx), _trunc(pjy)
        ix, iy, it = (np.zeros((n, 441), F) for _ in range(3))
        grad = (xi - 11 >= 0) & (xi + 11 < w) & (yi - 11 >= 0) & (yi + 11 < h)
        g = np.nonzero(grad)[0]
        if g.size:
            r, c = yi[g, None] + _DI[None], xi[g, None] + _DJ[None]
            ix[g] = (I[r, c + 1] - I[r, c - 1]) / F(2)
            iy[g] = (I[r + 1, c] - I[r - 1, c]) / F(2)
        timed = ((xi - 10 >= 0) & (xi + 10 < w) & (yi - 10 >= 0) & (yi + 10 < h) &
                 (xj - 10 >= 0) & (xj + 10 < w) & (yj - 10 >= 0) & (yj + 10 < h))
        t = np.nonzero(timed)[0]
        if t.size:
            it[t] = (J[yj[t, None] + _DI[None], xj[t, None] + _DJ[None]] -
                     I[yi[t, None] + _DI[None], xi[t, None] + _DJ[None]])
        sxx, syy, sxy = _seq_sum(ix * ix), _seq_sum(iy * iy), _seq_sum(ix * iy)
        sxt, syt = _seq_sum(ix * it), _seq_sum(iy * it)
        den = sxx * syy - sxy * sxy
        small = np.abs(den) < F(1e-9)
        status[small] = 3
        ok = ~small
        with np.errstate(all="ignore"):
            dx = ((F(-1) * syy) * sxt + sxy * syt) / den
            dy = ((F(-1) * sxx) * syt + sxt * sxy) / den
            pjx = np.where(ok, pjx + dx, pjx).astype(F)
            pjy = np.where(ok, pjy + dy, pjy).astype(F)
            if lv:
                pix, piy, pjx, pjy = pix * F(2), piy * F(2), pjx * F(2), pjy * F(2)
    return pjx, pjy, status


def lk_points(pyramids, points):
    """pyramids: {frame index: [level 0, 1, 2]} (the carry frame is -1); points: LK_POINT records.
    Returns the updated records."""
    out = np.array(points, LK_POINT).copy()
    flat = out.reshape(-1)
    x, y = flat["x"].copy(), flat["y"].copy()
    with np.errstate(invalid="ignore"):
        fine = (np.abs(x) < F(2.0 ** 24)) & (np.abs(y) < F(2.0 ** 24))
    active = flat["status"] == 0
    known = np.array([int(a) in pyramids and int(b) in pyramids
                      for a, b in zip(flat["frame_i"], flat["frame_j"])], bool).reshape(active.shape)
    bad = active & ~(fine & known)
    flat["status"][bad] = 3
    run = active & ~bad
    pairs = sorted({(int(a), int(b)) for a, b in zip(flat["frame_i"][run], flat["frame_j"][run])})
    for a, b in pairs:
        sel = np.nonzero(run & (flat["frame_i"] == a) & (flat["frame_j"] == b))[0]
        px, py, st = _lk_pair(pyramids[a], pyramids[b], x[sel], y[sel])
        flat["x"][sel], flat["y"][sel], flat["status"][sel] = px, py, st
    return out


# ---- matcher ----------------------------------------------------------------------------------
def match_threshold(distance, width, height):
    scaled = F(distance) * F(np.sqrt(np.float64(width * height))) / F(960)
    return F(10) if F(10) > scaled else scaled


def match_people(entries, entry_ids, people, size, next_id=0, inlier_ratio=INLIER_RATIO,
                 distance=DISTANCE):
    """entries [n, parts, 3], people [m, parts, 3] of (x, y, status); ascending entry_ids.
    Returns (ids int64 [m], next_id)."""
    people = np.asarray(people, F)
    entries = np.asarray(entries, F).reshape(-1, *people.shape[1:])
    entry_ids = [int(v) for v in entry_ids]
    m, n = people.shape[0], entries.shape[0]
    thr, ratio = match_threshold(distance, *size), F(inlier_ratio)
    ids = [-1] * m
    used = set()
    converged = False
    while m and not converged:
        cands, best, converged = [], F(0), True
        for i in range(m):
            if ids[i] != -1:
                continue
            for e in range(n):
                if e in used:
                    continue
                act = (entries[e, :, 2] == 0) & (people[i, :, 2] == 0)
                if not act.any():
                    continue
                dx = entries[e, act, 0] - people[i, act, 0]
                dy = entries[e, act, 1] - people[i, act, 1]
                with np.errstate(all="ignore"):
                    d = np.sqrt(dx * dx + dy * dy).astype(F)
                    total = _seq_sum(d[None])[0]
                    score = F(int((d < thr).sum())) / F(int(act.sum()))
                if score == best and score >= ratio:
                    cands.append((total, i, e))
                elif score > best and score >= ratio:
                    best, cands = score, [(total, i, e)]
        cands.sort(key=lambda c: (bool(np.isnan(c[0])), float(0 if np.isnan(c[0]) else c[0]),
                                  entry_ids[c[2]], c[1]))
        for _, i, e in cands:
            if e in used:
                continue
            ids[i] = entry_ids[e]
            used.add(e)
            converged = False
    for i in range(m):
        if ids[i] == -1:
            ids[i] = next_id
            next_id += 1
    return np.array(ids, np.int64).reshape(m), next_id


# ---- tracker ----------------------------------------------------------------------------------
class Tracker:
    """The strictly sequential oracle: one frame (a grey image) at a time."""

    def __init__(self, confidence=CONFIDENCE, inlier_ratio=INLIER_RATIO, distance=DISTANCE,
                 frames_to_delete=FRAMES_TO_DELETE):
        self.confidence, self.inlier_ratio, self.distance = F(confidence), inlier_ratio, distance
        self.frames_to_delete = frames_to_delete
        self.reset()

    def reset(self):
        self.next_id, self.entries, self.previous = 0, {}, None

    def frame(self, g, keypoints):
        """g: grey float32 [h, w]; keypoints [people, parts, 3] (x, y, score) -> ids int64."""
        kp = np.asarray(keypoints, F)
        kp = kp.reshape(-1, kp.shape[1] if kp.ndim == 3 else 1, 3)
        capture = kp.copy()
        capture[:, :, 2] = (kp[:, :, 2] < self.confidence).astype(F)
        current = pyramid(g, 3)
        if self.previous is None:
            for p in range(capture.shape[0]):
                self.entries[self.next_id] = [capture[p].copy(), 0]
                self.next_id += 1
        else:
            for key in sorted(self.entries):
                e = self.entries[key]
                counter, e[1] = e[1], e[1] + 1
                if counter > self.frames_to_delete:
                    del self.entries[key]
                    continue
                pts = np.zeros(e[0].shape[0], LK_POINT)
                pts["frame_i"], pts["frame_j"] = 0, 1
                pts["x"], pts["y"], pts["status"] = e[0][:, 0], e[0][:, 1], e[0][:, 2].astype(np.int32)
                out = lk_points({0: self.previous, 1: current}, pts)
                e[0] = np.stack([out["x"], out["y"], out["status"].astype(F)], axis=1).astype(F)
        keys = sorted(self.entries)
        ent = (np.stack([self.entries[k][0] for k in keys]) if keys
               else np.zeros((0,) + capture.shape[1:], F))
        ids, self.next_id = match_people(ent, keys, capture, (g.shape[1], g.shape[0]), self.next_id,
                                         self.inlier_ratio, self.distance)
        for p, key in enumerate(ids):
            self.entries[int(key)] = [capture[p].copy(), 0]
        self.previous = current
        return ids

    def run(self, greys, keypoints_list):
        return [self.frame(g, k) for g, k in zip(greys, keypoints_list)]


# ---- cases ------------------------------------------------------------------------------------
def texture(h, w, seed, cell=6):
    """A smooth uint8 BGR texture with gradients at every pyramid level."""
    rng = np.random.default_rng(seed)
    out = np.zeros((h, w, 3), np.float64)
    for c, amp in ((cell, 70.0), (3 * cell, 50.0)):
        gh, gw = h // c + 3, w // c + 3
        coarse = rng.uniform(-1, 1, (gh, gw, 3))
        yy, xx = np.arange(h) / c, np.arange(w) / c
        y0, x0 = yy.astype(int), xx.astype(int)
        fy, fx = (yy - y0)[:, None, None], (xx - x0)[None, :, None]
        a, b = coarse[y0][:, x0], coarse[y0][:, x0 + 1]
        cc, d = coarse[y0 + 1][:, x0], coarse[y0 + 1][:, x0 + 1]
        out += amp * ((a * (1 - fx) + b * fx) * (1 - fy) + (cc * (1 - fx) + d * fx) * fy)
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def lk_frames():
    """Three 192 x 128 BGR frames: a texture, the texture shifted by (+2, +1) pixels, a flat one."""
    big = texture(128 + 8, 192 + 8, seed=11)
    a = big[4:132, 4:196]
    b = big[3:131, 2:194]      # b[y][x] = a[y - 1][x - 2]
    flat = np.full_like(a, 90)
    return np.ascontiguousarray(np.stack([a, b, flat]))


def lk_grid(w=192, h=128):
    """The point records of the LK test: every pair of the edge coordinates, on frames 0 -> 1;
    the same coordinates against the flat frame; status-in 1; non-finite and huge coordinates."""
    xs = [-3.5, 0, 10.9, 11, 43.9, 44, 45.5, w - 45, w - 12, w - 11, w - 1, w + 5, 96, 77.25]
    ys = [-3.5, 0, 10.9, 11, 43.9, 44, 45.5, h - 45, h - 12, h - 11, h - 1, h + 5, 64, 70.75]
    rec = [(0, 1, x, y, 0) for y in ys for x in xs]
    rec += [(0, 2, x, 64, 0) for x in xs] + [(2, 1, 96, y, 0) for y in ys] + [(1, 0, 80.5, 60.25, 0)]
    rec += [(0, 1, 96, 64, 1), (0, 1, 50, 50, 2), (0, 1, np.inf, 64, 0), (0, 1, 96, -np.inf, 0),
            (0, 1, np.nan, 64, 0), (0, 1, 96, np.nan, 0), (0, 1, 3e7, 64, 0), (0, 1, 96, -3e7, 0),
            (0, 1, 2.0 ** 24, 64, 0), (0, 1, 16777215, 64, 0), (0, 3, 96, 64, 0), (-1, 1, 96, 64, 0)]
    return np.array(rec, LK_POINT)


SEQ_SIZE = (320, 240)
SEQ_FRAMES = 10
_RECTS = (((86, 105), (-2, 1)), ((160, 100), (1, 3)), ((232, 120), (2, -1)))   # centre, velocity
_HALF = (28, 40)                                                               # half width, height


def synthetic_sequence(seed=0, dropout=(1, (3, 4, 5))):
    """(frames uint8 [10, 240, 320, 3], keypoints per frame [people, 25, 3], truth per frame: which
    rectangle each person is).  Three textured rectangles moving 2-3 px per frame over a textured
    ground; 25 keypoints per rectangle on a 5 x 5 grid, jittered +-1 px, 3 of them below the
    confidence; the people shuffled per frame; rectangle dropout[0] undetected in frames dropout[1]."""
    w, h = SEQ_SIZE
    rng = np.random.default_rng(seed)
    ground = texture(h, w, seed=100 + seed)
    skins = [texture(2 * _HALF[1], 2 * _HALF[0], seed=200 + 10 * seed + r, cell=5) for r in range(3)]
    low = [rng.choice(25, 3, replace=False) for _ in range(3)]
    gx, gy = np.meshgrid(np.arange(-16, 17, 8), np.arange(-28, 29, 14))
    frames, keypoints, truth = [], [], []
    for f in range(SEQ_FRAMES):
        img = ground.copy()
        people = []
        for r, ((cx, cy), (vx, vy)) in enumerate(_RECTS):
            x0, y0 = cx + vx * f, cy + vy * f
            img[y0 - _HALF[1]:y0 + _HALF[1], x0 - _HALF[0]:x0 + _HALF[0]] = skins[r]
            kp = np.zeros((25, 3), np.float32)
            kp[:, 0] = x0 + gx.reshape(-1) + rng.integers(-1, 2, 25)
            kp[:, 1] = y0 + gy.reshape(-1) + rng.integers(-1, 2, 25)
            kp[:, 2] = 0.9
            kp[low[r], 2] = 0.05
            if not (r == dropout[0] and f in dropout[1]):
                people.append((r, kp))
        order = rng.permutation(len(people))
        frames.append(img)
        keypoints.append(np.stack([people[i][1] for i in order]) if people
                         else np.zeros((0, 25, 3), np.float32))
        truth.append([people[i][0] for i in order])
    return np.ascontiguousarray(np.stack(frames)), keypoints, truth


def stable_ids(ids_list, truth):
    """{rectangle: the set of ids it was given over the sequence}."""
    seen = {}
    for ids, who in zip(ids_list, truth):
        for i, r in zip(ids, who):
            seen.setdefault(r, set()).add(int(i))
    return seen
