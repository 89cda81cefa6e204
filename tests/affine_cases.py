"""Shared by the CPU and GPU tests of the affine and similarity estimators (psx_ransac_affine*, psx_ransac_similarity*,
psx_affine_fit, psx_similarity_fit, psx_ransac_samples_k with k = 2 and 3): an independent restatement of the rule of
csrc/hip/affine_rule.h, written from that header's comment -- python ints for the samples, numpy.float64 scalars under
np.errstate(all="ignore") for the fit (a zero divisor gives inf or NaN as IEEE does; plain python division raises), the
guide rule of tests/guided_cases.restate for the score -- and a generator of planted pair lists.

The restatement keeps L and D of the affine fit's factorisation in arrays of their own and the two right-hand sides as two
lists; the header factors in place.  The values are the same, the code is not.

scene(n, seed, kind): left positions uniform on 640 x 480.
  "similarity"  rotation 0.3 rad, scale 1.2, translation (25, -14)
  "affine"      the sheared matrix AFFINE_TRUE (a shear a similarity cannot represent)
  "shared"      the similarity, but every pair with p % 4 == 1 has the LEFT position of pair p - 1 (a keypoint that SIFT
                reports once per orientation): a sample that draws both is degenerate -- the 2-point fit divides by d = 0
                and gives NaN entries, which score 0
The right position of pair p is the transform of its left position plus an offset of radius ransac_cases.RADII[p % 3]
(0 / 0.5 / 1.5 px) at a random angle; when n > 4 every pair with p % 5 >= 3 is replaced
by a uniform outlier.  Both sides are rounded to float32.  The records index the position arrays through two permutations
and carry a payload in d1, d2.  tol = 2.
"""
import math

import numpy as np

from tests import guided_cases as gc
from tests.ransac_cases import (M32, PAIR_DTYPE, PAIR_U8_DTYPE, RADII, bits, correspondences, mix, same_records,  # noqa: F401
                                same_result)

TOL = 2.0
MIN = {"similarity": 2, "affine": 3}
MODELS = ("similarity", "affine")
SCENES = {"similarity": ("similarity", "shared"), "affine": ("affine", "shared")}
_C, _S = 1.2 * math.cos(0.3), 1.2 * math.sin(0.3)
SIMILARITY_TRUE = np.array([_C, -_S, 25.0, _S, _C, -14.0, 0.0, 0.0, 1.0])
AFFINE_TRUE = np.array([1.15, 0.32, -20.0, -0.08, 0.9, 31.0, 0.0, 0.0, 1.0])
TRUE = {"similarity": SIMILARITY_TRUE, "affine": AFFINE_TRUE, "shared": SIMILARITY_TRUE}


def shapes(model):
    """(n, N, seed): the edges of ransac_cases.SHAPES with the model's own minimum -- n = 0, MIN - 1, MIN and MIN + 1 (the
    last two are tie shapes), the ballot edge (63, 64, 65), 129 and 300, the single call's score block of 1024 pairs from
    both sides at N = 8, one case of several workgroups, N = 1 (the refit's own score launch), N = 65 and N = 257 (the
    select pass of 256)"""
    m = MIN[model]
    return [(0, 8, 0), (m - 1, 8, 0), (m, 8, 1), (m + 1, 64, 2), (63, 64, 3), (64, 65, 4), (65, 64, 5), (129, 257, 6), (300, 256, 7),
            (2500, 512, 8), (1023, 8, 9), (1024, 8, 9), (1025, 8, 32), (65, 1, 10)]


def tie_shapes(model):
    m = MIN[model]
    return [(m, 8, 1), (m + 1, 64, 2)]


def shape_id(shape):
    return "n%d_N%d" % shape[:2]


CASES = [(model, kind) + s for model in MODELS for kind in SCENES[model] for s in shapes(model)]
CASE_IDS = ["%s_%s_%s" % (model, kind, shape_id((n, N))) for model, kind, n, N, _ in CASES]


# ---- step 1 -----------------------------------------------------------------------------------------------------------
def samples(seed, h, n, k):
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
F64 = np.float64
ZERO, ONE = F64(0.0), F64(1.0)


def _columns(xy):
    a = np.asarray(xy, np.float32).reshape(-1, 2)
    return [F64(v) for v in a[:, 0]], [F64(v) for v in a[:, 1]]


def _side(xs, ys):
    """step 2a of one side: cx, cy, s and the normalised coordinates"""
    n = F64(len(xs))
    sx = sy = ZERO
    for x, y in zip(xs, ys):
        sx = sx + x
        sy = sy + y
    cx, cy = sx / n, sy / n
    d = ZERO
    for x, y in zip(xs, ys):
        d = d + (abs(x - cx) + abs(y - cy))
    s = n / d
    return cx, cy, s, [(x - cx) * s for x in xs], [(y - cy) * s for y in ys]


def _denormalise(rows, left, right):
    cxl, cyl, sl = left
    cxr, cyr, sr = right
    ir = ONE / sr
    out = []
    for (a, b, c), t in zip(rows, (cxr, cyr)):
        A, B = a * sl, b * sl
        Cc = (c - A * cxl) - B * cyl
        out += [A * ir, B * ir, Cc * ir + t]
    return np.array([np.float32(v) for v in out] + [np.float32(0), np.float32(0), np.float32(1)], np.float32)


def normalised_similarity(X, Y, U, V):
    """step 2b, SIMILARITY: the two normalised rows"""
    den = P = Q = ZERO
    for x, y, u, v in zip(X, Y, U, V):
        den = den + (x * x + y * y)
        P = P + (x * u + y * v)
        Q = Q + (x * v - y * u)
    p, q = P / den, Q / den
    return [(p, ZERO - q, ZERO), (q, p, ZERO)]


def normalised_affine(X, Y, U, V):
    """step 2b, AFFINE: the two normalised rows"""
    S = [[ZERO] * 3 for _ in range(3)]
    gu, gv = [ZERO] * 3, [ZERO] * 3
    for x, y, u, v in zip(X, Y, U, V):
        r = [x, y, ONE]
        for i in range(3):
            for j in range(i + 1):
                S[i][j] = S[i][j] + r[i] * r[j]
        for i in range(3):
            gu[i] = gu[i] + r[i] * u
            gv[i] = gv[i] + r[i] * v
    L = [[ZERO] * 3 for _ in range(3)]
    D = [ZERO] * 3
    for j in range(3):
        acc = ZERO
        for k in range(j):
            acc = acc + (L[j][k] * L[j][k]) * D[k]
        D[j] = S[j][j] - acc
        for i in range(j + 1, 3):
            acc = ZERO
            for k in range(j):
                acc = acc + (L[i][k] * L[j][k]) * D[k]
            L[i][j] = (S[i][j] - acc) / D[j]
    rows = []
    for g in (gu, gv):
        z = [ZERO] * 3
        for i in range(3):
            acc = ZERO
            for k in range(i):
                acc = acc + L[i][k] * z[k]
            z[i] = g[i] - acc
        w = [z[i] / D[i] for i in range(3)]
        q = [ZERO] * 3
        for i in (2, 1, 0):
            acc = ZERO
            for k in range(i + 1, 3):
                acc = acc + L[k][i] * q[k]
            q[i] = w[i] - acc
        rows.append(tuple(q))
    return rows


def fit(model, left_xy, right_xy):
    """the nine float32 entries fitted to left_xy[i] -> right_xy[i] (float32 positions), in the given order"""
    with np.errstate(all="ignore"):
        lx, ly = _columns(left_xy)
        rx, ry = _columns(right_xy)
        assert len(lx) == len(rx) >= MIN[model]
        cxl, cyl, sl, X, Y = _side(lx, ly)
        cxr, cyr, sr, U, V = _side(rx, ry)
        rows = (normalised_similarity if model == "similarity" else normalised_affine)(X, Y, U, V)
        return _denormalise(rows, (cxl, cyl, sl), (cxr, cyr, sr))


# ---- step 3 -----------------------------------------------------------------------------------------------------------
_BLOCK = 32


def passes(m, tol, pts):
    """bool per correspondence (pts: (n, 4) float32 xl, yl, xr, yr): the HOMOGRAPHY rule of guided matching as
    guided_cases.restate states it -- the diagonal of its relation, taken block by block -- and all False under a model
    with a non-finite entry"""
    m = np.asarray(m, np.float32).reshape(9)
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    out = np.zeros(len(pts), bool)
    if not np.isfinite(m).all():
        return out
    for a in range(0, len(pts), _BLOCK):
        blk = pts[a:a + _BLOCK]
        out[a:a + _BLOCK] = np.diagonal(gc.restate(gc.HOMOGRAPHY, m, tol, blk[:, 0:2], blk[:, 2:4]))
    return out


# ---- the whole rule -----------------------------------------------------------------------------------------------------
def _none(pairs, N):
    return dict(models=np.zeros((N, 9), np.float32), counts=np.zeros(N, np.int32), m=np.zeros(9, np.float32), best=-1,
                sample_inliers=0, inliers=0, refit_kept=0, records=pairs[:0])


def hypotheses(model, pairs, left_xy, right_xy, tol, N, seed):
    """steps 1 to 3 as the "no model" dict with models and counts filled in"""
    n, k = len(pairs), MIN[model]
    none = _none(pairs, N)
    if n < k:
        return none
    pts = correspondences(pairs, left_xy, right_xy)
    for h in range(N):
        idx = samples(seed, h, n, k)
        none["models"][h] = fit(model, pts[idx, 0:2], pts[idx, 2:4])
        none["counts"][h] = passes(none["models"][h], tol, pts).sum()
    return none


def finish(model, base, pairs, pts, tol, refit):
    """steps 4 to 6 on top of the hypotheses' models and counts"""
    models, counts = base["models"], base["counts"]
    best = int(np.argmax(counts))                                   # the first of the largest
    kept, sample_inliers, refit_kept = models[best].copy(), int(counts[best]), 0
    if refit and sample_inliers >= MIN[model]:
        sel = passes(kept, tol, pts)
        m2 = fit(model, pts[sel, 0:2], pts[sel, 2:4])
        if np.isfinite(m2).all() and passes(m2, tol, pts).sum() >= sample_inliers:
            kept, refit_kept = m2, 1
    if not np.isfinite(kept).all():
        return dict(base)
    sel = passes(kept, tol, pts)
    return dict(models=models, counts=counts, m=kept, best=best, sample_inliers=sample_inliers, inliers=int(sel.sum()),
                refit_kept=refit_kept, records=pairs[sel])


def ransac(model, pairs, left_xy, right_xy, tol, N, seed, refit):
    """dict: models (N, 9) float32, counts (N) int32, m (9), best, sample_inliers, inliers, refit_kept, records"""
    base = hypotheses(model, pairs, left_xy, right_xy, tol, N, seed)
    if len(pairs) < MIN[model]:
        return base
    return finish(model, base, pairs, correspondences(pairs, left_xy, right_xy), tol, refit)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def apply(m, p):
    """the transform of (n, 2) points under a matrix with last row (0, 0, 1), in double"""
    m = np.asarray(m, np.float64).reshape(3, 3)
    return np.asarray(p, np.float64) @ m[:2, :2].T + m[:2, 2]


def scene(n, seed, kind, noise=True):
    """(n, 4) float32 xl, yl, xr, yr and the planted mask; noise False: no offsets and no outliers"""
    rng = np.random.default_rng(13000 + seed)
    left = rng.uniform([0.0, 0.0], [640.0, 480.0], (n, 2))
    ang = rng.uniform(0.0, 2 * np.pi, n)
    out = rng.uniform([0.0, 0.0], [640.0, 480.0], (n, 2))
    if kind == "shared":
        for p in range(1, n, 4):
            left[p] = left[p - 1]
    right = apply(TRUE[kind], left)
    is_planted = np.ones(n, bool)
    if noise:
        rad = np.array([RADII[p % 3] for p in range(n)])
        right = right + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
        if n > 4:
            is_planted = (np.arange(n) % 5) < 3
            right[~is_planted] = apply(TRUE[kind], out)[~is_planted]
    return np.concatenate([left, right], 1).astype(np.float32), is_planted


_PLANTED = {}


def planted(n, seed, kind, u8=False):
    """(pairs, left_xy, right_xy, is_planted) of scene(n, seed, kind); read-only arrays, computed once"""
    key = (n, seed, kind, u8)
    if key not in _PLANTED:
        pts, is_planted = scene(n, seed, kind)
        rng = np.random.default_rng(15000 + seed)
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


def expect(model, kind, n, N, seed, refit):
    """the restatement's result on planted(n, seed, kind) at TOL, computed once (the hypotheses once for both refit
    settings)"""
    key = (model, kind, n, N, seed)
    pairs, lxy, rxy, _ = planted(n, seed, kind)
    if key not in _EXPECT:
        _EXPECT[key] = {None: hypotheses(model, pairs, lxy, rxy, TOL, N, seed)}
    e = _EXPECT[key]
    if refit not in e:
        e[refit] = dict(e[None]) if n < MIN[model] else finish(model, e[None], pairs, correspondences(pairs, lxy, rxy), TOL, refit)
    return e[refit]


def transfer(m, p):
    """where the (n, 2) points go under the float32 model m, in double (the model's own last row)"""
    m = np.asarray(m, np.float64).reshape(3, 3)
    q = np.concatenate([np.asarray(p, np.float64), np.ones((len(p), 1))], 1) @ m.T
    return q[:, :2] / q[:, 2:3]
