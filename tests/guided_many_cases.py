"""Shared by the CPU and GPU tests of the guided re-match of many sets (psx_match_pairs_guided_many_u8): the planted sets
of tests/match_many_cases.py with POSITIONS added in the manner of tests/guided_cases.positioned, a guide of its OWN for
every set, and the expected per-set lists derived without any device code.

Guides.  Set k takes entry k % 4 of: H_ASYM composed with a translation that grows with k (a homography, asymmetric in
its roles); F_EPI (the epipolar band through H_ASYM p); the all-admitting guide (identity, tol 1e30: the right-hand side
of the homography rule overflows to +inf); PSX_GUIDE_NONE (the set is skipped).

Positions.  The left points are uniform on a square canvas whose side gives a left point about 2.5 admissible right
points in the LARGEST homography-guided set (tol 2); left[1] -- planted_many's one-bit copy of left[0] -- sits 0.3 px from
left[0], so both find the copy of left[0] admissible and the cross-check has something to drop.  In set k the planted
partner of left point p sits at (the set's H) p plus an offset whose radius cycles through 0, 0.5, 1.5, 2.5 and 6 px (the
last two are inadmissible under the homography), the duplicate of the second planted row 1 px from its original's target
(an exact tie among admissible rights), every other right point uniform over the canvas' image.

Expected lists.  guided_cases.restate gives the relation A, guided_cases.expect_bytes_int64 the directed results in both
directions (A, then A transposed) from int64 distances, capi.pairs_join the host join."""
import numpy as np

from tests.guided_cases import EPIPOLAR, F_EPI, H_ASYM, HOMOGRAPHY, IDENTITY, MEAN_ADMISSIBLE, RADII, TOL, _apply_h, expect_bytes_int64, restate
from tests.match_many_cases import TINY_LENS, planted_many, tiny_many
from tests.match_pairs_cases import AMPS, assert_premise

NONE = 0
ALL_TOL = 1e30
# (seed, nl, right set lengths): the ballot step (63 / 64 / 65 / 129) and the backward block (255 / 256 / 257), empty and
# one-row sets; a long set between short ones; one left row; fewer left rows than one workgroup's four
CASES = [(31, 300, (257, 0, 1, 63, 64, 65, 129, 255, 256, 257)),
         (32, 257, (64, 1000, 300)),
         (33, 1, (1, 2, 40)),
         (34, 5, (3, 4, 5))]
CASE_IDS = ["seed%d" % c[0] for c in CASES]


def translated(h, tx, ty):
    """T(tx, ty) h: the homography h followed by a translation, row major float32"""
    t = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)
    return (t @ np.asarray(h, np.float64).reshape(3, 3)).astype(np.float32).reshape(9)


def guide_of(k):
    """(kind, m, tol) of set k"""
    which = k % 4
    if which == 0:
        return HOMOGRAPHY, translated(H_ASYM, 1.75 * k, -1.25 * k), TOL
    if which == 1:
        return EPIPOLAR, F_EPI, TOL
    if which == 2:
        return HOMOGRAPHY, IDENTITY, ALL_TOL
    return NONE, np.zeros(9, np.float32), 0.0


def placement_h(k):
    """the homography the positions of set k follow: its own guide's for a homography-guided set, H_ASYM otherwise"""
    kind, m, tol = guide_of(k)
    return m if k % 4 == 0 else H_ASYM


_POSITIONED = {}


def positioned_many(seed, nl, nrs):
    """(left, rights, left_xy, right_xys): planted_many(seed, nl, nrs) and float32 positions as the module docstring
    describes; computed once per case, read-only"""
    key = (seed, nl, tuple(nrs))
    if key in _POSITIONED:
        return _POSITIONED[key]
    left, rights = planted_many(seed, nl, nrs)
    h_lens = [n for k, n in enumerate(nrs) if k % 4 == 0] or list(nrs)
    side = max(4.0, float(np.sqrt(max(max(h_lens), 1) * np.pi * TOL * TOL / (1.5 * MEAN_ADMISSIBLE))))
    prng = np.random.default_rng([1000 + seed, 0])
    lxy = prng.uniform(0.0, side, (nl, 2))
    if nl >= 2:
        lxy[1] = lxy[0] + [0.3, 0.0]
    rxys = []
    for k, nr in enumerate(nrs):
        # the draws of planted_many(), repeated: which rows it paired (checked against the data below)
        rng = np.random.default_rng([seed, k + 1])
        rng.integers(0, 64, (nr, 128), dtype=np.uint8)
        m = min(nl, nr) // 2
        prng = np.random.default_rng([1000 + seed, k + 1])
        h = placement_h(k)
        corners = _apply_h(h, np.array([[0, 0], [side, 0], [0, side], [side, side]], np.float64))
        rxy = prng.uniform(corners.min(0), corners.max(0), (nr, 2))
        if m >= 1:
            src = np.concatenate([[0], 2 + rng.permutation(max(nl - 2, 0))]).astype(np.int64)[:m]
            dst = rng.permutation(nr)[:m]
            for t in range(m):
                diff = np.abs(left[src[t]].astype(np.int64) - rights[k][dst[t]].astype(np.int64))
                assert diff.max() <= max(AMPS), "tests/match_many_cases.planted_many draws differently than assumed here"
            ang = prng.uniform(0.0, 2 * np.pi, m)
            rad = np.array([RADII[t % len(RADII)] for t in range(m)])
            rxy[dst] = _apply_h(h, lxy[src]) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
            free = np.setdiff1d(np.arange(nr), dst)
            if m >= 2 and len(free):
                assert np.array_equal(rights[k][free[0]], rights[k][dst[1]])
                rxy[free[0]] = _apply_h(h, lxy[src[1:2]])[0] + [0.0, 1.0]
        rxys.append(rxy.astype(np.float32))
    lxy = lxy.astype(np.float32)
    for a in [left, lxy] + rights + rxys:
        a.setflags(write=False)
    _POSITIONED[key] = (left, rights, lxy, rxys)
    return _POSITIONED[key]


_DIRECTED = {}


def directed(key, left, lxy, right, rxy, guide):
    """(A, fm, fd, bm): the relation and the directed results L -> R under A and R -> L under A transposed, from int64
    distances alone; computed once per key"""
    if key not in _DIRECTED:
        kind, m, tol = guide
        A = restate(kind, m, tol, lxy, rxy)
        fm, fd = expect_bytes_int64(left, right, A)
        bm, _ = expect_bytes_int64(right, left, A.T)
        for a in (A, fm, fd, bm):
            a.setflags(write=False)
        _DIRECTED[key] = (A, fm, fd, bm)
    return _DIRECTED[key]


def wrong_backward(left, lxy, right, rxy, guide):
    """The backward result of an implementation that swaps the ROLES in the backward pass (the right point as the rule's
    left argument) instead of exchanging the loops"""
    kind, m, tol = guide
    W = restate(kind, m, tol, rxy, lxy)                   # W[j, i] = rule(left := right j, right := left i)
    return expect_bytes_int64(right, left, W)[0]


def expected(capi, case, k, ratio, mutual, guide_index=None, bwd=None):
    """The list the call owes for set k of case (seed, nl, nrs) under the guide of set guide_index (default: its own):
    PAIR_U8_DTYPE records.  bwd: a backward result to join with instead of the expected one (wrong_backward)."""
    seed, nl, nrs = case
    left, rights, lxy, rxys = positioned_many(*case)
    g = k if guide_index is None else guide_index
    guide = guide_of(g)
    if guide[0] == NONE or nl == 0 or nrs[k] == 0:
        return np.zeros(0, capi.PAIR_U8_DTYPE)
    A, fm, fd, bm = directed((seed, k, g), left, lxy, rights[k], rxys[k], guide)
    if bwd is not None:
        bm = bwd
    return capi.pairs_join(fm, fd, bm if mutual else None, nrs[k], ratio, mutual)


def premises(capi, case):
    """What makes the cases able to tell a wrong implementation from a right one; returns the number of sets per check"""
    seed, nl, nrs = case
    left, rights, lxy, rxys = positioned_many(*case)
    seen = dict(homography=0, swap=0, backward=0)
    for k, nr in enumerate(nrs):
        guide = guide_of(k)
        if guide[0] == NONE or min(nl, nr) < 64:
            continue
        own = expected(capi, case, k, 0.8, True)
        assert len(own) >= 1, (seed, k)
        for other in (k - 1, k + 1):                       # a wrong table index cannot pass
            if 0 <= other < len(nrs):
                swapped = expected(capi, case, k, 0.8, True, guide_index=other)
                assert own.tobytes() != swapped.tobytes(), (seed, k, other, "set k under a neighbour's guide gives the same list")
                seen["swap"] += 1
        if k % 4 != 0:
            continue
        A, fm, fd, bm = directed((seed, k, k), left, lxy, rights[k], rxys[k], guide)
        cnt = A.sum(1)
        assert (cnt == 0).any(), (seed, k, "no left row without an admissible right")
        assert (cnt == 1).any(), (seed, k, "no left row with exactly one admissible right")
        everything = np.ones_like(A)
        ub = expect_bytes_int64(left, rights[k], everything)[0][:, 0]
        lost = (~A[np.arange(nl), ub]) & (cnt >= 1)
        assert lost.any() and (fm[lost, 0] != ub[lost]).all(), (seed, k, "no unguided best that the guide excludes")
        assert_premise(fm, fd, bm, nr, (seed, k))          # kept / dropped by the ratio / dropped by the cross-check alone
        seen["homography"] += 1
        wb = wrong_backward(left, lxy, rights[k], rxys[k], guide)
        wrong = expected(capi, case, k, 0.8, True, bwd=wb)
        assert wrong.tobytes() != own.tobytes(), (seed, k, "roles swapped in the backward pass give the same list")
        seen["backward"] += 1
    return seen


def capi_guide(capi, guide):
    kind, m, tol = guide
    return capi.Guide.none() if kind == NONE else capi.Guide.make(kind, m, tol)


def tiny_guided(seed=35, nl=70):
    """tiny_many's 70 left rows and 200 sets of TINY_LENS with positions on a 12 x 12 canvas and a guide of its own per
    set: every fifth set kind 0, the others a window (identity + a translation that depends on k) of a radius that depends
    on k, or for k % 5 == 2 the epipolar band.  The exact copy of a left row in every non-empty set sits at its guide's
    image of that row, so every set that is not skipped yields a pair."""
    left, rights = tiny_many()
    rng = np.random.default_rng(seed)
    lxy = rng.uniform(0.0, 12.0, (nl, 2))
    guides, rxys = [], []
    for k, nr in enumerate(TINY_LENS):
        if k % 5 == 4:
            g, h = (NONE, np.zeros(9, np.float32), 0.0), IDENTITY
        elif k % 5 == 2:
            g, h = (EPIPOLAR, F_EPI, 1.0 + (k % 3)), H_ASYM
        else:
            h = translated(IDENTITY, 0.5 * (k % 7), -0.25 * (k % 11))
            g = (HOMOGRAPHY, h, 1.0 + 0.5 * (k % 4))
        corners = _apply_h(h, np.array([[0, 0], [12, 0], [0, 12], [12, 12]], np.float64))
        rxy = rng.uniform(corners.min(0), corners.max(0), (nr, 2))
        if nr:
            rxy[k % nr] = _apply_h(h, lxy[k % nl][None])[0]
        guides.append(g)
        rxys.append(rxy.astype(np.float32))
    return left, rights, lxy.astype(np.float32), rxys, guides
