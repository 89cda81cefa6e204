"""Shared by the CPU and GPU tests of the fundamental-matrix estimator (psx_ransac_fundamental*, psx_ransac_samples_k,
psx_fundamental_fit): an independent restatement of the rule of csrc/hip/fundamental_rule.h, written from that header's
comment -- python ints for the samples, python floats (IEEE double) for the fit, numpy float32 for the score -- and a
generator of two-view correspondences from a scene WITH DEPTH (a homography-planted set would leave F non-unique).

The restatement keeps the 9 x 9 matrix of step 2c as a full square array and exchanges whole rows and whole columns; the
header works on the lower triangle alone.  The values are the same, the code is not.

scene(n, seed, kind): left positions uniform on 640 x 480, depths uniform in [3, 9], camera K = (500, 500, 320, 240);
"general" rotates by 0.15 rad about y and translates by (-1, 0.1, 0.2); "rectified" is a pure sideways translation, for
which F is proportional to [0 0 0; 0 0 -1; 0 1 0] (the normalised F22 is exactly 0: the pivoting is exercised).  The right
position of pair p is its projection plus an offset of radius 0 / 0.5 / 1.5 px (p % 3) at a random angle; when n > 8 every
pair with p % 5 >= 3 is replaced by a uniform outlier.  Both sides are rounded to float32.  The records index the position
arrays through two permutations and carry a payload in d1, d2.  tol = 2.
"""
import math

import numpy as np

from tests.ransac_cases import (M32, PAIR_DTYPE, PAIR_U8_DTYPE, _div, _side, bits, correspondences, mix, same_records,  # noqa: F401
                                same_result)

TOL = 2.0
KINDS = ("general", "rectified")
# (n, N, seed): the ballot (64) and workgroup (256 pairs; 64 hypotheses per score workgroup, 256 per select pass)
# boundaries on both axes, below-minimum n, one case of several workgroups, the single call's score block of 1024 pairs
# (256 threads x 4 resident pairs) from both sides -- under (1025, 8, 32) the one pair of the second block passes under a
# hypothesis of either scene -- and N = 1, the hypothesis count of the refit's own score launch
SHAPES = [(0, 8, 0), (7, 8, 0), (8, 8, 1), (9, 64, 2), (63, 64, 3), (64, 65, 4), (65, 64, 5), (129, 128, 6), (300, 256, 7),
          (2500, 512, 8), (1023, 8, 9), (1024, 8, 9), (1025, 8, 32), (65, 1, 56)]
SHAPE_IDS = ["n%d_N%d" % (n, N) for n, N, _ in SHAPES]
TIE_SHAPES = [(8, 8, 1), (9, 64, 2)]


# ---- step 1 -----------------------------------------------------------------------------------------------------------
def samples(seed, h, n, k=8):
    base = mix((seed & M32) ^ ((0x9e3779b9 * (h + 1)) & M32))
    chosen = []
    for j in range(k):
        r = mix((base + j) & M32)
        idx = (r * (n - j)) >> 32
        for c in sorted(chosen):
            if idx >= c:
                idx += 1
        chosen.append(idx)
    return chosen


# ---- step 2 -----------------------------------------------------------------------------------------------------------
def _columns(xy):
    a = np.asarray(xy, np.float32).reshape(-1, 2)
    return [float(v) for v in a[:, 0]], [float(v) for v in a[:, 1]]


def fit(left_xy, right_xy, rounds=4, parts=False):
    """the nine float32 entries fitted to left_xy[i] -> right_xy[i] (float32 positions), in the given order.  rounds: the
    number of rank-correction rounds (the rule has 4).  parts: also the index of the free entry of step 2d"""
    lx, ly = _columns(left_xy)
    rx, ry = _columns(right_xy)
    assert len(lx) == len(rx) >= 8
    cxl, cyl, sl, X, Y = _side(lx, ly)
    cxr, cyr, sr, U, V = _side(rx, ry)
    # 2b
    S = [[0.0] * 9 for _ in range(9)]
    for x, y, u, v in zip(X, Y, U, V):
        r = [u * x, u * y, u, v * x, v * y, v, x, y, 1.0]
        for i in range(9):
            for j in range(i + 1):
                S[i][j] = S[i][j] + r[i] * r[j]
    for i in range(9):
        for j in range(i):
            S[j][i] = S[i][j]                                     # the full symmetric matrix
    # 2c
    perm = list(range(9))
    for j in range(8):
        p = j
        for i in range(j + 1, 9):
            if abs(S[i][i]) > abs(S[p][p]):
                p = i
        if p != j:
            S[j], S[p] = S[p], S[j]                               # rows (the finished columns 0..j-1 go with them)
            for row in S:
                row[j], row[p] = row[p], row[j]                   # columns
            perm[j], perm[p] = perm[p], perm[j]
        l = [0.0] * 9
        for i in range(j + 1, 9):
            l[i] = _div(S[i][j], S[j][j])
        for i in range(j + 1, 9):
            for k in range(j + 1, i + 1):
                S[i][k] = S[i][k] - l[i] * S[k][j]
                S[k][i] = S[i][k]
        for i in range(j + 1, 9):
            S[i][j] = l[i]
    # 2d
    q = [0.0] * 9
    q[8] = 1.0
    for i in range(7, -1, -1):
        acc = 0.0
        for k in range(i + 1, 9):
            acc = acc + S[k][i] * q[k]
        q[i] = 0.0 - acc
    F = [0.0] * 9
    for i in range(9):
        F[perm[i]] = q[i]
    # 2e
    for _ in range(rounds):
        C = [F[4] * F[8] - F[5] * F[7], F[5] * F[6] - F[3] * F[8], F[3] * F[7] - F[4] * F[6],
             F[2] * F[7] - F[1] * F[8], F[0] * F[8] - F[2] * F[6], F[1] * F[6] - F[0] * F[7],
             F[1] * F[5] - F[2] * F[4], F[2] * F[3] - F[0] * F[5], F[0] * F[4] - F[1] * F[3]]
        det = (F[0] * C[0] + F[1] * C[1]) + F[2] * C[2]
        nn = 0.0
        for k in range(9):
            nn = nn + C[k] * C[k]
        t = _div(det, nn)
        F = [F[k] - t * C[k] for k in range(9)]
    # 2f
    G = []
    for r in range(3):
        a, b, c = F[3 * r:3 * r + 3]
        A, B = a * sl, b * sl
        G.append([A, B, (c - A * cxl) - B * cyl])
    row0 = [G[0][k] * sr for k in range(3)]
    row1 = [G[1][k] * sr for k in range(3)]
    row2 = [(G[2][k] - cxr * row0[k]) - cyr * row1[k] for k in range(3)]
    with np.errstate(all="ignore"):
        m = np.array([np.float32(v) for v in row0 + row1 + row2], np.float32)
    return (m, perm[8]) if parts else m


# ---- step 3 -----------------------------------------------------------------------------------------------------------
def usable(m):
    m = np.asarray(m, np.float32).reshape(9)
    return bool(np.isfinite(m).all() and m.any())


def passes(m, tol, pts):
    """bool per correspondence (pts: (n, 4) float32 xl, yl, xr, yr): the EPIPOLAR rule of guided matching, elementwise,
    every float32 operation rounded on its own; all False under a model that is not usable (a non-finite entry, or all
    nine zero)"""
    f = np.float32
    m = np.asarray(m, f).reshape(9)
    pts = np.asarray(pts, f).reshape(-1, 4)
    if not usable(m):
        return np.zeros(len(pts), bool)
    tol = f(tol)
    xl, yl, xr, yr = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
    with np.errstate(all="ignore"):
        a = (m[0] * xl + m[1] * yl) + m[2]
        b = (m[3] * xl + m[4] * yl) + m[5]
        c = (m[6] * xl + m[7] * yl) + m[8]
        e = (a * xr + b * yr) + c
        lhs, rhs = e * e, (tol * tol) * (a * a + b * b)
        assert lhs.dtype == f and rhs.dtype == f
        return lhs <= rhs


# ---- the whole rule -----------------------------------------------------------------------------------------------------
def _finish(base, pairs, pts, tol, refit):
    """steps 5 and 6 on top of the hypotheses' models and counts"""
    models, counts = base["models"], base["counts"]
    best = int(np.argmax(counts))                                   # the first of the largest
    kept, sample_inliers, refit_kept = models[best].copy(), int(counts[best]), 0
    if refit and sample_inliers >= 8:
        sel = passes(kept, tol, pts)
        m2 = fit(pts[sel, 0:2], pts[sel, 2:4])
        if usable(m2) and passes(m2, tol, pts).sum() >= sample_inliers:
            kept, refit_kept = m2, 1
    if not usable(kept):
        return dict(base)
    sel = passes(kept, tol, pts)
    return dict(models=models, counts=counts, m=kept, best=best, sample_inliers=sample_inliers, inliers=int(sel.sum()),
                refit_kept=refit_kept, records=pairs[sel])


def hypotheses(pairs, left_xy, right_xy, tol, N, seed):
    """steps 1 to 3 as the "no model" dict with models and counts filled in"""
    n = len(pairs)
    none = dict(models=np.zeros((N, 9), np.float32), counts=np.zeros(N, np.int32), m=np.zeros(9, np.float32), best=-1,
                sample_inliers=0, inliers=0, refit_kept=0, records=pairs[:0])
    if n < 8:
        return none
    pts = correspondences(pairs, left_xy, right_xy)
    for h in range(N):
        idx = samples(seed, h, n)
        none["models"][h] = fit(pts[idx, 0:2], pts[idx, 2:4])
        none["counts"][h] = passes(none["models"][h], tol, pts).sum()
    return none


def ransac(pairs, left_xy, right_xy, tol, N, seed, refit):
    """dict: models (N, 9) float32, counts (N) int32, m (9), best, sample_inliers, inliers, refit_kept, records"""
    base = hypotheses(pairs, left_xy, right_xy, tol, N, seed)
    if len(pairs) < 8:
        return base
    return _finish(base, pairs, correspondences(pairs, left_xy, right_xy), tol, refit)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def scene(n, seed, kind):
    """(n, 4) float32 xl, yl, xr, yr and the planted mask"""
    rng = np.random.default_rng(7000 + seed)
    K = np.array([[500., 0, 320], [0, 500., 240], [0, 0, 1]])
    if kind == "general":
        a = 0.15
        R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        t = np.array([-1.0, 0.1, 0.2])
    else:
        assert kind == "rectified"
        R = np.eye(3)
        t = np.array([-0.5, 0, 0])
    left = rng.uniform([0, 0], [640, 480], (n, 2))
    z = rng.uniform(3, 9, n)
    X = np.linalg.inv(K) @ np.concatenate([left, np.ones((n, 1))], 1).T * z
    xr = K @ (R @ X + t[:, None])
    right = (xr[:2] / xr[2]).T
    ang = rng.uniform(0, 2 * np.pi, n)
    rad = np.array([(0., .5, 1.5)[p % 3] for p in range(n)])
    right = right + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    planted = np.ones(n, bool)
    if n > 8:
        planted = (np.arange(n) % 5) < 3
        out = rng.uniform([0, 0], [640, 480], (n, 2))
        right[~planted] = out[~planted]
    return np.concatenate([left, right], 1).astype(np.float32), planted


_PLANTED = {}


def planted(n, seed, kind, u8=False):
    """(pairs, left_xy, right_xy, is_planted) of scene(n, seed, kind); read-only arrays, computed once"""
    key = (n, seed, kind, u8)
    if key not in _PLANTED:
        pts, is_planted = scene(n, seed, kind)
        rng = np.random.default_rng(9000 + seed)
        lperm, rperm = rng.permutation(n), rng.permutation(n)
        lxy = np.zeros((n, 2), np.float32)
        rxy = np.zeros((n, 2), np.float32)
        lxy[lperm] = pts[:, 0:2]
        rxy[rperm] = pts[:, 2:4]
        pairs = np.zeros(n, PAIR_U8_DTYPE if u8 else PAIR_DTYPE)
        pairs["left"], pairs["right"] = lperm, rperm
        pairs["d1"] = np.arange(n) + 1
        pairs["d2"] = 2 * np.arange(n) + 7
        for a in (pairs, lxy, rxy, is_planted):
            a.setflags(write=False)
        _PLANTED[key] = (pairs, lxy, rxy, is_planted)
    return _PLANTED[key]


_EXPECT = {}


def expect(n, N, seed, kind, refit):
    """the restatement's result on planted(n, seed, kind) at TOL, computed once (the hypotheses once for both refit settings)"""
    key = (n, N, seed, kind)
    pairs, lxy, rxy, _ = planted(n, seed, kind)
    if key not in _EXPECT:
        _EXPECT[key] = {None: hypotheses(pairs, lxy, rxy, TOL, N, seed)}
    e = _EXPECT[key]
    if refit not in e:
        e[refit] = dict(e[None]) if n < 8 else _finish(e[None], pairs, correspondences(pairs, lxy, rxy), TOL, refit)
    return e[refit]


def conditioned_rank_ratio(m):
    """sigma3 / sigma1 of the model after conditioning both images by x -> x / 320 - 1, y -> y / 240 - 1"""
    T = np.array([[1 / 320., 0, -1], [0, 1 / 240., -1], [0, 0, 1]])
    Ti = np.linalg.inv(T)
    s = np.linalg.svd(Ti.T @ np.asarray(m, np.float64).reshape(3, 3) @ Ti, compute_uv=False)
    return s[2] / s[0]


_CHAIN = {}


def chain_case(n=200, seed=11):
    """(left, right, left_xy, right_xy): float32 descriptor sets planted on the "general" scene's positions for the chain
    match -> verify -> guided re-match.  Point p of the scene is left row p and right row perm[p]; the right descriptor of
    every planted point, and of every second outlier (a confident match at the wrong place: what verification is for), is
    its left descriptor plus noise of amplitude 2 .. 8; the other outliers' right descriptors are unrelated."""
    key = (n, seed)
    if key not in _CHAIN:
        pts, is_planted = scene(n, seed, "general")
        rng = np.random.default_rng(11000 + seed)
        left = rng.integers(0, 64, (n, 128), dtype=np.uint8)
        right = rng.integers(0, 64, (n, 128), dtype=np.uint8)
        perm = rng.permutation(n)
        for p in range(n):
            if is_planted[p] or p % 2 == 0:
                amp = (2, 4, 8)[p % 3]
                right[perm[p]] = np.clip(left[p].astype(np.int64) + rng.integers(-amp, amp + 1, 128), 0, 255).astype(np.uint8)
        rxy = np.zeros((n, 2), np.float32)
        rxy[perm] = pts[:, 2:4]
        out = (left.astype(np.float32), right.astype(np.float32), np.ascontiguousarray(pts[:, 0:2]), rxy, is_planted, perm)
        for a in out:
            a.setflags(write=False)
        _CHAIN[key] = out
    return _CHAIN[key]
