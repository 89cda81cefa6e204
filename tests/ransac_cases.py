"""Shared by the CPU and GPU tests of geometric verification (psx_ransac_homography*, psx_ransac_samples,
psx_homography_fit): an independent restatement of the rule of csrc/hip/ransac_rule.h, written from that header's comment
-- python ints for the samples, python floats (IEEE double) for the fit, numpy float32 for the score -- and a generator of
planted pair lists.

Planted input of n pairs (seed s): left positions uniform on 640 x 480; the right position of pair p is guided_cases.H_ASYM
applied to its left position plus an offset of radius 0 / 0.5 / 1.5 px (p % 3) at a random angle; when n > 4 every pair with
p % 5 >= 3 is replaced by a uniform outlier on the image of the canvas.  Both sides are rounded to float32.  The records
index the position arrays through two permutations and carry a payload in d1, d2 (the inlier list must copy records whole).
tol = 2: every planted pair is an inlier of the true model.
"""
import math

import numpy as np

from tests.guided_cases import H_ASYM

TOL = 2.0
RADII = (0.0, 0.5, 1.5)
# (n, N, seed): the ballot (64) and workgroup (256 pairs; 64 hypotheses per score workgroup, 256 per select pass)
# boundaries on both axes, below-minimum n, one case of several workgroups, the single call's score block of 1024 pairs
# (256 threads x 4 resident pairs) from both sides, and N = 1, the hypothesis count of the refit's own score launch
SHAPES = [(0, 8, 0), (3, 8, 0), (4, 8, 1), (5, 64, 2), (63, 64, 3), (64, 65, 4), (65, 64, 5), (129, 128, 6), (300, 256, 7),
          (2500, 512, 8), (1023, 8, 9), (1024, 8, 9), (1025, 8, 32), (65, 1, 10)]
SHAPE_IDS = ["n%d_N%d" % (n, N) for n, N, _ in SHAPES]
TIE_SHAPES = [(4, 8, 1), (5, 64, 2)]
PAIR_DTYPE = np.dtype([("left", "<i4"), ("right", "<i4"), ("d1", "<f4"), ("d2", "<f4")])
PAIR_U8_DTYPE = np.dtype([("left", "<i4"), ("right", "<i4"), ("d1", "<i4"), ("d2", "<i4")])

M32 = 0xffffffff


# ---- step 1 -----------------------------------------------------------------------------------------------------------
def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def samples(seed, h, n):
    base = mix((seed & M32) ^ ((0x9e3779b9 * (h + 1)) & M32))
    chosen = []
    for k in range(4):
        r = mix((base + k) & M32)
        idx = (r * (n - k)) >> 32
        for c in sorted(chosen):
            if idx >= c:
                idx += 1
        chosen.append(idx)
    return chosen


# ---- step 2 -----------------------------------------------------------------------------------------------------------
def _div(a, b):
    """IEEE double division: what ZeroDivisionError stands for is the IEEE result (NaN for 0 / 0, else a signed inf)"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _side(xs, ys):
    n = float(len(xs))
    sx = sy = 0.0
    for x, y in zip(xs, ys):
        sx = sx + x
        sy = sy + y
    cx, cy = _div(sx, n), _div(sy, n)
    d = 0.0
    for x, y in zip(xs, ys):
        d = d + (abs(x - cx) + abs(y - cy))
    s = _div(n, d)
    return cx, cy, s, [(x - cx) * s for x in xs], [(y - cy) * s for y in ys]


def fit(left_xy, right_xy):
    """the nine float32 entries fitted to left_xy[i] -> right_xy[i] (float32 positions), in the given order"""
    lx = [float(v) for v in np.asarray(left_xy, np.float32).reshape(-1, 2)[:, 0]]
    ly = [float(v) for v in np.asarray(left_xy, np.float32).reshape(-1, 2)[:, 1]]
    rx = [float(v) for v in np.asarray(right_xy, np.float32).reshape(-1, 2)[:, 0]]
    ry = [float(v) for v in np.asarray(right_xy, np.float32).reshape(-1, 2)[:, 1]]
    assert len(lx) == len(rx) >= 4
    cxl, cyl, sl, X, Y = _side(lx, ly)
    cxr, cyr, sr, U, V = _side(rx, ry)
    S = [[0.0] * 8 for _ in range(8)]
    g = [0.0] * 8
    for x, y, u, v in zip(X, Y, U, V):
        for r, t in (([x, y, 1.0, 0.0, 0.0, 0.0, -(u * x), -(u * y)], u), ([0.0, 0.0, 0.0, x, y, 1.0, -(v * x), -(v * y)], v)):
            for i in range(8):
                for j in range(i + 1):
                    S[i][j] = S[i][j] + r[i] * r[j]
                g[i] = g[i] + r[i] * t
    L = [[0.0] * 8 for _ in range(8)]
    D = [0.0] * 8
    for j in range(8):
        acc = 0.0
        for k in range(j):
            acc = acc + (L[j][k] * L[j][k]) * D[k]
        D[j] = S[j][j] - acc
        for i in range(j + 1, 8):
            acc = 0.0
            for k in range(j):
                acc = acc + (L[i][k] * L[j][k]) * D[k]
            L[i][j] = _div(S[i][j] - acc, D[j])
    z = [0.0] * 8
    for i in range(8):
        acc = 0.0
        for k in range(i):
            acc = acc + L[i][k] * z[k]
        z[i] = g[i] - acc
    w = [_div(z[i], D[i]) for i in range(8)]
    q = [0.0] * 8
    for i in range(7, -1, -1):
        acc = 0.0
        for k in range(i + 1, 8):
            acc = acc + L[k][i] * q[k]
        q[i] = w[i] - acc
    hn = q + [1.0]
    G = []
    for r in range(3):
        a, b, c = hn[3 * r:3 * r + 3]
        A, B = a * sl, b * sl
        G.append([A, B, (c - A * cxl) - B * cyl])
    ir = _div(1.0, sr)
    H = [G[0][k] * ir + cxr * G[2][k] for k in range(3)] + [G[1][k] * ir + cyr * G[2][k] for k in range(3)] + G[2]
    with np.errstate(all="ignore"):
        return np.array([np.float32(v) for v in H], np.float32)


# ---- step 3 -----------------------------------------------------------------------------------------------------------
def passes(m, tol, pts):
    """bool per correspondence (pts: (n, 4) float32 xl, yl, xr, yr): the HOMOGRAPHY rule of guided matching, elementwise,
    every float32 operation rounded on its own; all False under a model with a non-finite entry"""
    f = np.float32
    m = np.asarray(m, f).reshape(9)
    pts = np.asarray(pts, f).reshape(-1, 4)
    if not np.isfinite(m).all():
        return np.zeros(len(pts), bool)
    tol = f(tol)
    xl, yl, xr, yr = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
    with np.errstate(all="ignore"):
        a = (m[0] * xl + m[1] * yl) + m[2]
        b = (m[3] * xl + m[4] * yl) + m[5]
        c = (m[6] * xl + m[7] * yl) + m[8]
        dx, dy = a - c * xr, b - c * yr
        tc = tol * c
        lhs, rhs = dx * dx + dy * dy, tc * tc
        assert lhs.dtype == f and rhs.dtype == f
        return (c > f(0)) & (lhs <= rhs)


def correspondences(pairs, left_xy, right_xy):
    lx, rx = np.asarray(left_xy, np.float32).reshape(-1, 2), np.asarray(right_xy, np.float32).reshape(-1, 2)
    return np.concatenate([lx[pairs["left"]], rx[pairs["right"]]], 1).reshape(-1, 4)


# ---- the whole rule -----------------------------------------------------------------------------------------------------
def ransac(pairs, left_xy, right_xy, tol, N, seed, refit):
    """dict: models (N, 9) float32, counts (N) int32, m (9), best, sample_inliers, inliers, refit_kept, records"""
    n = len(pairs)
    none = dict(models=np.zeros((N, 9), np.float32), counts=np.zeros(N, np.int32), m=np.zeros(9, np.float32), best=-1,
                sample_inliers=0, inliers=0, refit_kept=0, records=pairs[:0])
    if n < 4:
        return none
    pts = correspondences(pairs, left_xy, right_xy)
    models = np.zeros((N, 9), np.float32)
    counts = np.zeros(N, np.int32)
    for h in range(N):
        idx = samples(seed, h, n)
        models[h] = fit(pts[idx, 0:2], pts[idx, 2:4])
        counts[h] = passes(models[h], tol, pts).sum()
    best = int(np.argmax(counts))                                   # the first of the largest
    kept, sample_inliers, refit_kept = models[best].copy(), int(counts[best]), 0
    if refit and sample_inliers >= 4:
        sel = passes(kept, tol, pts)
        m2 = fit(pts[sel, 0:2], pts[sel, 2:4])
        if np.isfinite(m2).all() and passes(m2, tol, pts).sum() >= sample_inliers:
            kept, refit_kept = m2, 1
    if not np.isfinite(kept).all():
        return dict(none, models=models, counts=counts)
    sel = passes(kept, tol, pts)
    return dict(models=models, counts=counts, m=kept, best=best, sample_inliers=sample_inliers, inliers=int(sel.sum()),
                refit_kept=refit_kept, records=pairs[sel])


# ---- planted inputs -----------------------------------------------------------------------------------------------------
def _apply_h(m, p):
    m = np.asarray(m, np.float64).reshape(3, 3)
    q = np.concatenate([p, np.ones((len(p), 1))], 1) @ m.T
    return q[:, :2] / q[:, 2:3]


_PLANTED = {}


def planted(n, seed, u8=False):
    """(pairs, left_xy, right_xy, is_planted): see the module docstring; read-only arrays, computed once"""
    key = (n, seed, u8)
    if key not in _PLANTED:
        rng = np.random.default_rng(5000 + seed)
        left = rng.uniform([0.0, 0.0], [640.0, 480.0], (n, 2))
        ang = rng.uniform(0.0, 2 * np.pi, n)
        rad = np.array([RADII[p % 3] for p in range(n)])
        right = _apply_h(H_ASYM, left) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
        corners = _apply_h(H_ASYM, np.array([[0, 0], [640, 0], [0, 480], [640, 480]], np.float64))
        outlier = rng.uniform(corners.min(0), corners.max(0), (n, 2))
        is_planted = np.ones(n, bool)
        if n > 4:
            is_planted = (np.arange(n) % 5) < 3
            right[~is_planted] = outlier[~is_planted]
        lperm, rperm = rng.permutation(n), rng.permutation(n)
        lxy = np.zeros((n, 2), np.float32)
        rxy = np.zeros((n, 2), np.float32)
        lxy[lperm] = left.astype(np.float32)
        rxy[rperm] = right.astype(np.float32)
        pairs = np.zeros(n, PAIR_U8_DTYPE if u8 else PAIR_DTYPE)
        pairs["left"], pairs["right"] = lperm, rperm
        pairs["d1"] = np.arange(n) + 1
        pairs["d2"] = 2 * np.arange(n) + 7
        for a in (pairs, lxy, rxy, is_planted):
            a.setflags(write=False)
        _PLANTED[key] = (pairs, lxy, rxy, is_planted)
    return _PLANTED[key]


_EXPECT = {}


def expect(n, N, seed, refit):
    """the restatement's result on planted(n, seed) at TOL, computed once"""
    key = (n, N, seed, refit)
    if key not in _EXPECT:
        pairs, lxy, rxy, _ = planted(n, seed)
        if refit and (n, N, seed, False) in _EXPECT:                # the hypotheses are the same: only the refit is new
            base = _EXPECT[(n, N, seed, False)]
            _EXPECT[key] = _refit_of(base, pairs, lxy, rxy)
        else:
            _EXPECT[key] = ransac(pairs, lxy, rxy, TOL, N, seed, refit)
    return _EXPECT[key]


def _refit_of(base, pairs, lxy, rxy):
    if base["best"] < 0 or base["sample_inliers"] < 4:
        return dict(base)
    pts = correspondences(pairs, lxy, rxy)
    sel = passes(base["m"], TOL, pts)
    m2 = fit(pts[sel, 0:2], pts[sel, 2:4])
    if np.isfinite(m2).all() and passes(m2, TOL, pts).sum() >= base["sample_inliers"]:
        sel2 = passes(m2, TOL, pts)
        return dict(base, m=m2, refit_kept=1, inliers=int(sel2.sum()), records=pairs[sel2])
    return dict(base)


def bits(a):
    """float32 arrays as comparable 32-bit patterns, every NaN (whatever its sign or payload) as one value"""
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def same_result(res, want):
    """a RansacResult (or any object with m, best, sample_inliers, inliers, refit_kept) against a restatement dict"""
    return (np.array_equal(bits(np.array(list(res.m), np.float32)), bits(want["m"])) and res.best == want["best"] and
            res.sample_inliers == want["sample_inliers"] and res.inliers == want["inliers"] and res.refit_kept == want["refit_kept"])


def same_records(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return len(a) == len(b) and a.dtype.itemsize == b.dtype.itemsize == 16 and np.array_equal(a.view(np.int32), b.view(np.int32))
