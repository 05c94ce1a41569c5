"""3-D keypoints from a camera rig: the numpy restatement of the include/opk.h text ("3-D keypoints
from a camera rig"), a LAPACK variant of it, and seeded case builders.

The restatement works on plain Python floats (IEEE fp64, every operation rounded on its own) with
sequential sums -- no np.dot, no np.hypot, no power operator -- so it is the text, operation by
operation.  The LAPACK variant is the same flow with the null vector of A taken from
numpy.linalg.svd: an independent implementation of the one step the text had to restate (the
reference takes it from cv::SVD).
"""
import math

import numpy as np

F32 = np.float32
DBL_EPSILON = 2.220446049250313e-16
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
NAN = float("nan")


def _div(a, b):
    """IEEE a / b (Python raises on a zero divisor)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 or a != a else NAN


def camera_matrix(K, Rt):
    """K [3][3] x Rt [3][4], every entry a sequential sum over k."""
    out = np.zeros((3, 4), np.float64)
    for i in range(3):
        for j in range(4):
            s = 0.0
            for k in range(3):
                s = s + float(K[i][k]) * float(Rt[k][j])
            out[i, j] = s
    return out


def effective_min_views(min_views, V):
    return min_views if min_views > 0 else max(2, min(4, V - 1))


def max_acceptable(sizes):
    w0h0 = int(sizes[0][0]) * int(sizes[0][1])
    return 25 * _sqrt(w0h0 / 1310720.)


def valid(k, size):
    """isValidKeypoint, in float32 against the int bounds."""
    x, y, s = F32(k[0]), F32(k[1]), F32(k[2])
    return bool(s > F32(0.35) and x > F32(8) and x < F32(int(size[0]) - 8) and y > F32(8)
                and y < F32(int(size[1]) - 8))


def build_A(P, xs, ys, S):
    V = len(P)
    A = [[0.0] * 4 for _ in range(2 * V)]
    for i in range(V):
        if i not in S:
            continue
        for k in range(4):
            A[2 * i][k] = xs[i] * P[i][2][k] - P[i][0][k]
            A[2 * i + 1][k] = ys[i] * P[i][2][k] - P[i][1][k]
    return A


def jacobi_null(A):
    """The null vector by cyclic one-sided Jacobi; returns (v, sweeps used, ended by convergence)."""
    rows = len(A)
    A = [r[:] for r in A]
    Vm = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    W = [0.0] * 4
    for i in range(4):
        w = 0.0
        for k in range(rows):
            w = w + A[k][i] * A[k][i]
        W[i] = w
    sweeps, converged = 0, False
    for _ in range(30):
        sweeps += 1
        changed = False
        for i, j in PAIRS:
            p = 0.0
            for k in range(rows):
                p = p + A[k][i] * A[k][j]
            if abs(p) <= DBL_EPSILON * _sqrt(W[i] * W[j]):
                continue
            p = p * 2.0
            beta = W[i] - W[j]
            gamma = _sqrt(p * p + beta * beta)
            if beta < 0.0:
                delta = (gamma - beta) * 0.5
                s = _sqrt(_div(delta, gamma))
                c = _div(p, gamma * s * 2.0)
            else:
                c = _sqrt(_div(gamma + beta, gamma * 2.0))
                s = _div(p, gamma * c * 2.0)
            wi = wj = 0.0
            for k in range(rows):
                t0 = c * A[k][i] + s * A[k][j]
                t1 = c * A[k][j] - s * A[k][i]
                A[k][i], A[k][j] = t0, t1
                wi = wi + t0 * t0
                wj = wj + t1 * t1
            W[i], W[j] = wi, wj
            for k in range(4):
                t0 = c * Vm[k][i] + s * Vm[k][j]
                t1 = c * Vm[k][j] - s * Vm[k][i]
                Vm[k][i], Vm[k][j] = t0, t1
            changed = True
        if not changed:
            converged = True
            break
    m, wm = 0, W[0]
    for i in range(1, 4):
        if W[i] < wm:
            wm, m = W[i], i
    return [Vm[k][m] for k in range(4)], sweeps, converged


def lapack_null(A):
    with np.errstate(all="ignore"):
        _, _, vh = np.linalg.svd(np.array(A, np.float64))
    return [float(x) for x in vh[-1]], 0, True


def solve(P, xs, ys, S, null=jacobi_null, info=None):
    """ONE TRIANGULATION over the views S (ascending): (X [4], error)."""
    v, sweeps, converged = null(build_A(P, xs, ys, S))
    if info is not None:
        info["max_sweeps"] = max(info.get("max_sweeps", 0), sweeps)
        info["unconverged"] = info.get("unconverged", 0) + (0 if converged else 1)
    X = [_div(v[k], v[3]) for k in range(4)]
    total = 0.0
    for i in S:
        r = []
        for j in range(3):
            a = 0.0
            for k in range(4):
                a = a + P[i][j][k] * X[k]
            r.append(a)
        dx = _div(r[0], r[2]) - xs[i]
        dy = _div(r[1], r[2]) - ys[i]
        total = total + _sqrt(dx * dx + dy * dy)
    return X, _div(total, float(len(S)))


def _near(value, threshold, info):
    """Notes an error within a relative 1e-9 of a threshold it is compared with."""
    if info is not None and value == value and threshold == threshold and \
            abs(value - threshold) <= 1e-9 * abs(threshold):
        info["near"] = info.get("near", 0) + 1


def point(P, xs, ys, S, max_acc, null=jacobi_null, info=None):
    """ONE POINT: (X, error, dropped view or -1)."""
    X, e = solve(P, xs, ys, S, null, info)
    dropped = -1
    _near(e, 0.5 * max_acc, info)
    if len(S) >= 4 and e > 0.5 * max_acc:
        best = e
        for i in S:
            Xi, ei = solve(P, xs, ys, [v for v in S if v != i], null, info)
            _near(ei, 0.9 * e, info)
            if best > ei and ei < 0.9 * e:
                best, dropped, X = ei, i, Xi
        e = best
    return X, e, dropped


def reconstruct(P, sizes, min_views, keypoints, present=None, null=jacobi_null, info=None):
    """The whole call: keypoints [steps][V][parts][3], present [steps][V].  Returns xyz float32
    [steps][parts][4], status int32 [steps], errors float64 [steps][parts] (-1: not attempted),
    dropped int32 [steps][parts]; info (a dict, optional) gains max_sweeps, unconverged, near, and
    x64 = the fp64 points of the attempted parts, keyed (step, part)."""
    P = [[[float(e) for e in row] for row in m] for m in np.asarray(P, np.float64)]
    V = len(P)
    kp = np.asarray(keypoints, np.float32)
    steps, _, parts, _ = kp.shape
    present = np.ones((steps, V), np.int32) if present is None else np.asarray(present)
    mv = effective_min_views(min_views, V)
    max_acc = max_acceptable(sizes)
    xyz = np.zeros((steps, parts, 4), np.float32)
    status = np.zeros(steps, np.int32)
    errors = np.full((steps, parts), -1.0, np.float64)
    dropped = np.full((steps, parts), -1, np.int32)
    with np.errstate(all="ignore"):
        for t in range(steps):
            if int(np.count_nonzero(present[t])) < 2:
                continue
            cand = {}
            for p in range(parts):
                S = [i for i in range(V) if present[t][i] and valid(kp[t, i, p], sizes[i])]
                if len(S) < mv:
                    continue
                xs = [float(kp[t, i, p, 0]) for i in range(V)]
                ys = [float(kp[t, i, p, 1]) for i in range(V)]
                X, e, d = point(P, xs, ys, S, max_acc, null, info)
                cand[p] = (F32(X[0]), F32(X[1]), F32(X[2]))
                errors[t, p] = e
                dropped[t, p] = d
                if info is not None:
                    info.setdefault("x64", {})[(t, p)] = X[:3]
            if not cand:
                continue
            status[t] = 1
            total = 0.0
            for p in sorted(cand):
                total = total + float(errors[t, p])
            total = _div(total, float(len(cand)))
            for p in sorted(cand):
                e = float(errors[t, p])
                _near(e, 5 * total, info)
                _near(e, max_acc, info)
                x, y, z = cand[p]
                if np.isfinite(x) and np.isfinite(y) and np.isfinite(z) and e < 5 * total \
                        and e < max_acc:
                    xyz[t, p] = (x, y, z, 1)
    return xyz, status, errors, dropped


# ---- case builders ------------------------------------------------------------------------------
def ring_rig(rng, V, size=(1280, 720)):
    """V cameras on a ring looking at the origin, K of 900-1400 px focal length: (P [V][3][4],
    sizes [V][2])."""
    P = np.zeros((V, 3, 4), np.float64)
    start = rng.uniform(0, 2 * math.pi)
    for i in range(V):
        a = start + 2 * math.pi * i / V + rng.uniform(-0.2, 0.2)
        C = np.array([rng.uniform(3.5, 5.5) * math.cos(a), rng.uniform(-0.6, 0.6),
                      rng.uniform(3.5, 5.5) * math.sin(a)])
        z = -C / np.linalg.norm(C)
        x = np.cross(np.array([0., 1., 0.]), z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        f = rng.uniform(900, 1400)
        K = np.array([[f, 0, size[0] / 2], [0, f * rng.uniform(0.98, 1.02), size[1] / 2], [0, 0, 1]])
        P[i] = camera_matrix(K, np.concatenate([R, (-R @ C)[:, None]], 1))
    return P, np.array([size] * V, np.int32)


def plane_rig(V, size, depth=3.0, offset=0.4):
    """V cameras with distinct centres that all map the plane z = depth to the same pixels, up to
    a shift of offset * v px in view v: the same (x, y) detected in every view is then a point of
    that plane, seen with reprojection errors of a fraction of a pixel.  P_v = T_v (P_0 + a_v pi^T)
    with P_0 = K [I | 0], pi = (0, 0, 1, -depth) the plane and T_v the shift.  (P [V][3][4],
    sizes [V][2]).  For tests whose views are copies of one frame."""
    K = np.array([[600., 0, size[0] / 2], [0, 600., size[1] / 2], [0, 0, 1]])
    P0 = camera_matrix(K, np.eye(3, 4))
    plane = np.array([0., 0., 1., -depth])
    P = np.zeros((V, 3, 4), np.float64)
    for v in range(V):
        a = K @ np.array([0.3 * v, 0.1 * v * (-1) ** v, 0.0])
        T = np.array([[1., 0, offset * v], [0, 1., -0.75 * offset * v], [0, 0, 1]])
        P[v] = T @ (P0 + np.outer(a, plane))
    return P, np.array([size] * V, np.int32)


def project(P, X):
    """[V][2] pixel positions of the 3-D point X."""
    h = np.asarray(P) @ np.append(np.asarray(X, np.float64), 1.0)
    return h[:, :2] / h[:, 2:3]


def scene(rng, P, steps, parts, noise=0.0, spread=0.35, score=0.9):
    """keypoints float32 [steps][V][parts][3] of random points around the origin, every view's
    detection noised by N(0, noise) px; also the points [steps][parts][3]."""
    V = len(P)
    pts = rng.uniform(-spread, spread, (steps, parts, 3))
    kp = np.zeros((steps, V, parts, 3), np.float32)
    for t in range(steps):
        for p in range(parts):
            uv = project(P, pts[t, p]) + (rng.normal(0, noise, (V, 2)) if noise else 0.0)
            kp[t, :, p, :2] = uv
            kp[t, :, p, 2] = score
    return kp, pts


def ulp_apart(a, b):
    """The largest distance in float32 ulps between two float32 arrays of finite values."""
    a = np.asarray(a, np.float32).ravel()
    b = np.asarray(b, np.float32).ravel()
    if a.size == 0:
        return 0.0
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))
    # np.spacing at a power of two is the ulp above it; a step down across it is half of that
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / sp))
