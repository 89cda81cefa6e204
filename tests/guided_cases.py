"""Shared by the CPU and GPU tests of guided matching (psx_match_guided*, psx_match_pairs_guided*, psx_guide_allows):
the planted descriptor sets of tests/match_pairs_cases.py with POSITIONS added, two guides, an independent numpy float32
restatement of the admissibility rule, and the expected directed results derived from the oracle.

Positions.  Left points are uniform on a small square canvas, sized from the right side's length so that a left point
has about 2.5 admissible right points under the homography guide (H_ASYM, tol 2).  The planted partner of a left point p
sits at H p plus an offset whose radius cycles through 0, 0.5, 1.5, 2.5 and 6 px (the last two are inadmissible); every
other right point is uniform over the canvas' image under H.  Two deliberate placements make the premises below hold
whatever the seed: the copy of the duplicated right row sits 1 px from H p of the same left point as its original (both
copies inside the tolerance: an exact tie among admissible rights), and left rows 5 and 6 -- copies of the first planted
source row -- sit 0.3 px from it, so the three left rows that want the same right row all find it admissible and the
cross-check has something to drop.  The epipolar guide F_EPI = [e]x H_ASYM (rank 2) is used on the same points: the line of
a left point p passes through H p.

Expected values.  A = restated relation (nl x nr bool).  For left i the expected row is oracle.match(left[i], right[A_i])
with indices mapped back through the ascending A_i (so ties keep the smaller original index); zero or one admissible
right are written out here: (0, 0, reject, inf, inf) and (j, 0, accept, d, inf).  Backward: the same with A transposed."""
import numpy as np

from tests.match_pairs_cases import AMPS, INT_MAX, assert_premise, dist_as_int, planted

TOL = 2.0
RADII = (0.0, 0.5, 1.5, 2.5, 6.0)
MEAN_ADMISSIBLE = 2.5
# scale about 1.25 / 1.2, a small shear and perspective, a translation; c > 0 over every canvas used here
H_ASYM = np.array([1.25, 0.03, 4.0, -0.02, 1.2, -3.0, 1e-4, -5e-5, 1.0], np.float32)
_E = np.array([-60.0, 35.0, 1.0])
_EX = np.array([[0.0, -_E[2], _E[1]], [_E[2], 0.0, -_E[0]], [-_E[1], _E[0], 0.0]])
F_EPI = (_EX @ H_ASYM.astype(np.float64).reshape(3, 3) / 64.0).astype(np.float32).reshape(9)
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)

HOMOGRAPHY, EPIPOLAR = 1, 2
GUIDES = {"homography": (HOMOGRAPHY, H_ASYM, TOL), "epipolar": (EPIPOLAR, F_EPI, TOL)}

# the named sets: (nl, nr, seed); the premises are asserted on each (tests/test_match_guided_cpu.py)
NAMED = {"300x257": (300, 257, 1), "257x513": (257, 513, 2), "64x1000": (64, 1000, 3)}
# every directed shape of the GPU tests: the named ones, small and empty sides, and the ballot step boundary (63 / 64 /
# 65 / 129 inner points against 70 outer ones)
SHAPES = [(33, 31, 8), (300, 257, 1), (257, 513, 2), (64, 1000, 3), (1, 1, 4), (129, 1, 5), (5, 0, 6), (0, 7, 7),
          (70, 63, 21), (70, 64, 22), (70, 65, 23), (70, 129, 24)]
SHAPE_IDS = ["%dx%d" % (a, b) for a, b, _ in SHAPES]


def restate(kind, m, tol, left_xy, right_xy):
    """The rule of include/popsift_hip.h ("guided matching") in numpy float32, independent of the library: every operation
    rounded on its own, in the documented order.  Returns the (nl, nr) bool relation."""
    f = np.float32
    m = np.asarray(m, f).reshape(9)
    tol = f(tol)
    lx, rx = np.asarray(left_xy, f).reshape(-1, 2), np.asarray(right_xy, f).reshape(-1, 2)
    xl, yl = lx[:, 0][:, None], lx[:, 1][:, None]
    xr, yr = rx[:, 0][None, :], rx[:, 1][None, :]
    with np.errstate(all="ignore"):
        a = (m[0] * xl + m[1] * yl) + m[2]
        b = (m[3] * xl + m[4] * yl) + m[5]
        c = (m[6] * xl + m[7] * yl) + m[8]
        if kind == HOMOGRAPHY:
            dx, dy = a - c * xr, b - c * yr
            tc = tol * c
            lhs, rhs = dx * dx + dy * dy, tc * tc
            assert lhs.dtype == f and rhs.dtype == f
            out = (c > f(0)) & (lhs <= rhs)
        else:
            e = (a * xr + b * yr) + c
            lhs, rhs = e * e, (tol * tol) * (a * a + b * b)
            assert lhs.dtype == f and rhs.dtype == f
            out = lhs <= rhs
    return np.broadcast_to(out, (len(lx), len(rx))).copy()


def _apply_h(m, p):
    m = np.asarray(m, np.float64).reshape(3, 3)
    q = np.concatenate([p, np.ones((len(p), 1))], 1) @ m.T
    return q[:, :2] / q[:, 2:3]


def positioned(seed, nl, nr):
    """(left, right, left_xy, right_xy): planted(seed, nl, nr) and float32 positions as the module docstring describes"""
    left, right = planted(seed, nl, nr)
    # the draws of planted(), repeated: which rows it paired (checked against the data below)
    rng = np.random.default_rng(seed)
    rng.integers(0, 64, (nl, 128), dtype=np.uint8)
    rng.integers(0, 64, (nr, 128), dtype=np.uint8)
    k = min(nl, nr) // 2
    src = dst = np.zeros(0, np.int64)
    if k >= 1:
        rows = np.arange(nl) if nl <= 6 else np.setdiff1d(np.arange(nl), [5, 6])
        src = rng.permutation(rows)[:k]
        dst = rng.permutation(nr)[:k]
        for t in range(k):
            diff = np.abs(left[src[t]].astype(np.int64) - right[dst[t]].astype(np.int64))
            assert diff.max() <= max(AMPS), "tests/match_pairs_cases.planted draws differently than assumed here"
    prng = np.random.default_rng(1000 + seed)
    # canvas side: nr * (pi tol^2) / (area of the canvas' image, ~1.5 S^2) = MEAN_ADMISSIBLE
    side = max(4.0, float(np.sqrt(max(nr, 1) * np.pi * TOL * TOL / (1.5 * MEAN_ADMISSIBLE))))
    lxy = prng.uniform(0.0, side, (nl, 2))
    corners = _apply_h(H_ASYM, np.array([[0, 0], [side, 0], [0, side], [side, side]], np.float64))
    lo, hi = corners.min(0), corners.max(0)
    rxy = prng.uniform(lo, hi, (nr, 2))
    if k >= 1:
        if nl > 6:
            lxy[5] = lxy[src[0]] + [0.3, 0.0]
            lxy[6] = lxy[src[0]] + [0.0, -0.3]
        ang = prng.uniform(0.0, 2 * np.pi, k)
        rad = np.array([RADII[t % len(RADII)] for t in range(k)])
        rxy[dst] = _apply_h(H_ASYM, lxy[src]) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
        free = np.setdiff1d(np.arange(nr), dst)
        if k >= 2 and len(free):
            assert np.array_equal(right[free[0]], right[dst[1]])
            rxy[free[0]] = _apply_h(H_ASYM, lxy[src[1:2]])[0] + [0.0, 1.0]
    lxy, rxy = lxy.astype(np.float32), rxy.astype(np.float32)
    for a in (left, right, lxy, rxy):
        a.setflags(write=False)
    return left, right, lxy, rxy


def expect_directed(oracle, left, right, A, u8):
    """The expected guided directed result of `left` against `right` under the relation A (len(left) x len(right)):
    (match (n, 3) int32, dist (n, 2) float32, or int32 with INT_MAX for +inf when u8)"""
    lf, rf = np.asarray(left, np.float32).reshape(-1, 128), np.asarray(right, np.float32).reshape(-1, 128)
    n = len(lf)
    mm = np.zeros((n, 3), np.int32)
    dd = np.full((n, 2), np.inf, np.float32)
    for i in range(n):
        idx = np.nonzero(A[i])[0]                         # ascending
        if len(idx) == 0:
            continue                                      # no neighbour: indices 0, +inf twice, inf / inf is NaN: rejected
        m, d = oracle.match(lf[i:i + 1], rf[idx])
        if len(idx) == 1:
            assert np.isfinite(d[0, 0])
            mm[i] = (idx[0], 0, 1)                        # one neighbour: second index 0 at +inf, d / inf = 0 < 0.8: accepted
            dd[i] = (d[0, 0], np.inf)
            continue
        mm[i] = (idx[m[0, 0]], idx[m[0, 1]], m[0, 2])
        dd[i] = d[0]
    if u8:
        dd = dist_as_int(dd)
    return mm, dd


def expect_bytes_int64(left, right, A):
    """The same for bytes from integer squared distances in numpy int64 alone -- no oracle: the two smallest under
    (distance, index) order among the admissible rights"""
    l, r = np.asarray(left, np.int64).reshape(-1, 128), np.asarray(right, np.int64).reshape(-1, 128)
    n = len(l)
    mm = np.zeros((n, 3), np.int32)
    dd = np.full((n, 2), INT_MAX, np.int32)
    for i in range(n):
        idx = np.nonzero(A[i])[0]
        if len(idx) == 0:
            continue
        d = ((r[idx] - l[i]) ** 2).sum(1)
        order = np.lexsort((idx, d))[:2]
        mm[i, 0], dd[i, 0] = idx[order[0]], d[order[0]]
        if len(order) > 1:
            mm[i, 1], dd[i, 1] = idx[order[1]], d[order[1]]
        f1 = np.float32(dd[i, 0])
        f2 = np.float32(np.inf) if dd[i, 1] == INT_MAX else np.float32(dd[i, 1])
        with np.errstate(all="ignore"):
            mm[i, 2] = 1 if f1 / f2 < np.float32(0.8) else 0
    return mm, dd


_CASES = {}


def case(oracle, seed, nl, nr, guide, u8):
    """Everything the tests need of one (set, guide, format), computed once: dict with left, right (uint8 or float32),
    lxy, rxy, kind, m, tol, A, and the expected directed results fm, fd (L -> R under A), bm, bd (R -> L under A
    transposed)"""
    key = (seed, nl, nr, guide, u8)
    if key not in _CASES:
        left, right, lxy, rxy = positioned(seed, nl, nr)
        kind, m, tol = GUIDES[guide]
        A = restate(kind, m, tol, lxy, rxy)
        fm, fd = expect_directed(oracle, left, right, A, u8)
        bm, bd = expect_directed(oracle, right, left, A.T, u8)
        l = left if u8 else left.astype(np.float32)
        r = right if u8 else right.astype(np.float32)
        for a in (A, fm, fd, bm, bd, l, r):
            a.setflags(write=False)
        _CASES[key] = dict(left=l, right=r, lxy=lxy, rxy=rxy, kind=kind, m=m, tol=tol, A=A, fm=fm, fd=fd, bm=bm, bd=bd)
    return _CASES[key]


def wrong_backward(oracle, c, u8):
    """The backward result of an implementation that swaps the ROLES in the backward pass (evaluates the rule with the right
    point as its left argument) instead of exchanging the loops: what the asymmetric H must tell apart"""
    W = restate(c["kind"], c["m"], c["tol"], c["rxy"], c["lxy"])          # W[j, i] = rule(left := right j, right := left i)
    return expect_directed(oracle, c["right"], c["left"], W, u8)


def premises(oracle, c, what, admissible_counts=True):
    """The seven premises of a named set, from the oracle-derived expectation alone.  admissible_counts: also 1 and 2 (a
    left descriptor with no / exactly one admissible right), which only the homography guide's canvas is sized for."""
    A, fm, fd, bm = c["A"], c["fm"], c["fd"], c["bm"]
    cnt = A.sum(1)
    if admissible_counts:
        assert (cnt == 0).any(), (what, "no left descriptor without an admissible right")
        assert (cnt == 1).any(), (what, "no left descriptor with exactly one admissible right")
    um, _ = oracle.match(np.asarray(c["left"], np.float32), np.asarray(c["right"], np.float32))
    ub = um[:, 0]
    lost = (~A[np.arange(len(A)), ub]) & (cnt >= 1)
    assert lost.any() and (fm[lost, 0] != ub[lost]).all(), (what, "no unguided best that the guide excludes")
    tie = (cnt >= 2) & (fd[:, 0] == fd[:, 1])
    assert tie.any(), (what, "no exact tie among admissible rights")
    assert_premise(fm, fd, bm, len(c["right"]), what)              # kept / dropped by the ratio / dropped by the cross-check alone
    return dict(mean_admissible=float(cnt.mean()), none=int((cnt == 0).sum()), one=int((cnt == 1).sum()),
                lost=int(lost.sum()), ties=int(tie.sum()))
