"""Shared by tests/test_rule_edges_cpu.py and tests/test_gpu_rule_edges.py: inputs that sit ON the comparisons of the
rules host and device share (csrc/hip/guide_rule.h, match_rule.h, kp_place.h) and on the boundaries of the walk around
the guide rule (k_match_guided).  Nothing here needs a GPU or the library; what needs the oracle takes it as an argument.

1. probe_set(guide): per guide of guided_cases.GUIDES, N = 1024 primary left points p uniform in [0, 60]^2.  Each has
   two PROBE rights placed, in float64, exactly on the boundary of its admissible set -- homography: H p + tol (cos, sin)
   at two angles 120 to 240 degrees apart; epipolar: on the line of p, tol along its normal on either side -- rounded to
   float32, and then the x coordinate moved by a seeded step of -6 .. +6 float32 ulps.  About half are admitted, and a
   device copy that contracts a multiply-add, or compares with '<', decides hundreds of them differently.
   Every probe r also gets a FALLBACK left p' = H^-1 r: H p' is the probe itself (homography), the line of p' passes
   through it (epipolar, F = [e]x H), so (p', r) is firmly admissible.  Lefts = primaries and fallbacks (3 N), rights = probes
   (2 N), both in a seeded permutation.
   Descriptors (bytes; the float sets are the same integers).  Primary i holds a random row B_i of values in [64, 192); its
   probes are B_i moved by exact squared distances d_a < d_b, both below 20, on disjoint components; the fallback of a probe
   is the probe's row moved by 10 in one further component (squared distance 100 to its probe, more to the other).  Random
   rows are some 3e5 apart.  So the forward top-2 of primary i shows both probe decisions whatever else the band admits,
   and with PSX_PAIRS_MUTUAL at ratio inf the pair (i, probe) is kept iff both passes admit it while (p', probe) is kept iff
   the BACKWARD pass rejects (i, probe).
2. walk_calls() / tie_call() / nonfinite_calls(): identity H, tol 0.25, positions on an integer lattice: a pair is admissible
   iff the two points coincide, so the set bits of every ballot step are chosen one by one, nowhere near the comparison.
3. ratio_set(): planted sets with exactly known integer (d1, d2) per left row, and the ratios on and next to each quotient.
4. boundary_records() / position_edge_records(): keypoint records on the tables of automatic placement and on the borders.
5. the special-value point and guide lists of the guide rule, and two constructions that make the device's WHOLE relation
   visible: right slices of two rows (forward) and a diagonal set with fallbacks (backward)."""
import math

import numpy as np

from tests import guided_cases as gc
from tests.match_pairs_cases import INT_MAX, dist_as_int

F32 = np.float32


# ---- small helpers --------------------------------------------------------------------------------------------------------
def squares(d, cap=60):
    """d >= 0 as a list of integers <= cap whose squares sum to d (greedy, largest first)"""
    out, d = [], int(d)
    while d > 0:
        s = min(cap, math.isqrt(d))
        out.append(s)
        d -= s * s
    return out


def moved(row, d, comps):
    """a copy of the integer row at exact squared distance d from it, the difference spread over the components `comps`"""
    row = np.asarray(row, np.int64).copy()
    sq = squares(d)
    assert len(sq) <= len(comps), (d, len(sq))
    for c, s in zip(comps, sq):
        row[c] += s
    assert row.min() >= 0 and row.max() <= 255
    return row


def int_distances(left, right):
    """exact squared distances of integer-valued rows, int64 (n, m)"""
    l, r = np.asarray(left, np.float64).reshape(-1, 128), np.asarray(right, np.float64).reshape(-1, 128)
    d = (l * l).sum(1)[:, None] + (r * r).sum(1)[None, :] - 2.0 * (l @ r.T)          # integers far below 2^53: exact
    return np.rint(d).astype(np.int64)


def top2(D, A, u8):
    """guided_cases.expect_directed / expect_bytes_int64 for integer-valued rows, vectorised: the two smallest under
    (distance, index) order among the admissible columns of the int64 distance matrix D; (match (n, 3) int32, dist (n, 2)
    int32 with INT_MAX, or float32 with +inf)"""
    n, m = D.shape
    mm = np.zeros((n, 3), np.int32)
    dd = np.full((n, 2), INT_MAX, np.int64)
    none = np.int64(1) << 62
    if n and m:
        key = np.where(A, D * (1 << 20) + np.arange(m, dtype=np.int64)[None, :], none)
        rows = np.arange(n)
        for s in range(min(2, m)):
            j = key.argmin(1)
            ok = key[rows, j] < none
            mm[ok, s] = j[ok]
            dd[ok, s] = D[rows, j][ok]
            key[rows, j] = none
    f = np.where(dd == INT_MAX, np.inf, dd).astype(F32)
    with np.errstate(all="ignore"):
        mm[:, 2] = f[:, 0] / f[:, 1] < F32(0.8)
    return mm, (dd.astype(np.int32) if u8 else f)


def as_format(rows, u8):
    rows = np.asarray(rows)
    return np.ascontiguousarray(rows.astype(np.uint8 if u8 else np.float32))


def step_ulps(v, k):
    """float32 array v moved by k[i] float32 ulps (k integer, either sign)"""
    v = np.asarray(v, F32).copy()
    k = np.asarray(k)
    for _ in range(int(np.abs(k).max()) if len(k) else 0):
        up, dn = k > 0, k < 0
        v[up] = np.nextafter(v[up], F32(np.inf))
        v[dn] = np.nextafter(v[dn], F32(-np.inf))
        k = k - np.sign(k)
    return v


# ---- 1. the guide rule at its comparison ------------------------------------------------------------------------------------
def restate_contracted(kind, m, tol, left_xy, right_xy):
    """guided_cases.restate with every x*y + z of the rule contracted to one fused multiply-add: product plus addend in
    float64 (the product of two float32 is exact there), rounded once to float32.  What a device build without
    -ffp-contract=off may compute."""
    f = F32
    m = np.asarray(m, f).reshape(9)
    tol = f(tol)
    lx, rx = np.asarray(left_xy, f).reshape(-1, 2), np.asarray(right_xy, f).reshape(-1, 2)
    xl, yl = lx[:, 0][:, None], lx[:, 1][:, None]
    xr, yr = rx[:, 0][None, :], rx[:, 1][None, :]
    d = np.float64

    def fma(x, y, z):
        return (np.asarray(x, d) * np.asarray(y, d) + np.asarray(z, d)).astype(f)

    with np.errstate(all="ignore"):
        a = fma(m[0], xl, m[1] * yl) + m[2]
        b = fma(m[3], xl, m[4] * yl) + m[5]
        c = fma(m[6], xl, m[7] * yl) + m[8]
        if kind == gc.HOMOGRAPHY:
            dx, dy = fma(-c, xr, a), fma(-c, yr, b)
            tc = tol * c
            out = (c > f(0)) & (fma(dx, dx, dy * dy) <= tc * tc)
        else:
            e = fma(a, xr, b * yr) + c
            out = e * e <= (tol * tol) * fma(a, a, b * b)
    return np.broadcast_to(out, (len(lx), len(rx))).copy()


PROBE_N = 1024
PROBE_SEEDS = {"homography": 101, "epipolar": 202}
_PROBES = {}


def _apply(M, p):
    q = np.concatenate([p, np.ones((len(p), 1))], 1) @ M.T
    return q[:, :2] / q[:, 2:3]


def probe_set(guide, n=PROBE_N):
    """dict: left, right (uint8 rows), lxy, rxy (float32), kind, m, tol, A (restated relation), and the index arrays prim
    (n), probe (n, 2), fall (n, 2): left index of primary i, right indices of its two probes, left indices of their
    fallbacks"""
    key = (guide, n)
    if key in _PROBES:
        return _PROBES[key]
    kind, m, tol = gc.GUIDES[guide]
    rng = np.random.default_rng(PROBE_SEEDS[guide])
    H = gc.H_ASYM.astype(np.float64).reshape(3, 3)
    p = rng.uniform(0.0, 60.0, (n, 2)).astype(F32)
    p64 = p.astype(np.float64)
    hp = _apply(H, p64)
    if kind == gc.HOMOGRAPHY:
        th = rng.uniform(0.0, 2 * np.pi, n)
        th2 = th + rng.uniform(2 * np.pi / 3, 4 * np.pi / 3, n)
        pr = [hp + tol * np.stack([np.cos(t), np.sin(t)], 1) for t in (th, th2)]
    else:
        ln = np.concatenate([p64, np.ones((n, 1))], 1) @ np.asarray(m, np.float64).reshape(3, 3).T
        nrm = np.hypot(ln[:, 0], ln[:, 1])
        nv = ln[:, :2] / nrm[:, None]
        tv = np.stack([-nv[:, 1], nv[:, 0]], 1)
        foot = hp - ((ln[:, 0] * hp[:, 0] + ln[:, 1] * hp[:, 1] + ln[:, 2]) / nrm)[:, None] * nv
        pr = [foot + rng.uniform(-20.0, 20.0, n)[:, None] * tv + sgn * tol * nv for sgn in (1.0, -1.0)]
    probes = []
    for q in pr:
        q = q.astype(F32)
        q[:, 0] = step_ulps(q[:, 0], rng.integers(-6, 7, n))
        probes.append(q)
    Hinv = np.linalg.inv(H)
    falls = [_apply(Hinv, q.astype(np.float64)).astype(F32) for q in probes]
    # descriptors
    B = rng.integers(64, 192, (n, 128)).astype(np.int64)
    da = rng.integers(1, 10, n)
    db = da + rng.integers(1, 10, n)
    ra = np.stack([moved(B[i], da[i], (0, 1, 2, 3)) for i in range(n)])
    rb = np.stack([moved(B[i], db[i], (8, 9, 10, 11)) for i in range(n)])
    fa, fb = ra.copy(), rb.copy()
    fa[:, 20] += 10
    fb[:, 21] += 10
    lperm, rperm = rng.permutation(3 * n), rng.permutation(2 * n)
    left = np.concatenate([B, fa, fb])[lperm].astype(np.uint8)
    lxy = np.concatenate([p, falls[0], falls[1]])[lperm]
    right = np.concatenate([ra, rb])[rperm].astype(np.uint8)
    rxy = np.concatenate(probes)[rperm]
    linv, rinv = np.argsort(lperm), np.argsort(rperm)
    prim = linv[:n]
    fall = np.stack([linv[n:2 * n], linv[2 * n:]], 1)
    probe = np.stack([rinv[:n], rinv[n:]], 1)
    A = gc.restate(kind, m, tol, lxy, rxy)
    out = dict(left=left, right=right, lxy=np.ascontiguousarray(lxy), rxy=np.ascontiguousarray(rxy), kind=kind, m=m, tol=tol,
               A=A, prim=prim, probe=probe, fall=fall, da=da, db=db)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _PROBES[key] = out
    return out


_EXPECTED = {}


def expected(oracle, key, left, right, A):
    """guided_cases.expect_directed both ways, once per key, for integer-valued rows: dict u8 -> (fm, fd, bm, bd)"""
    if key not in _EXPECTED:
        fm, fd = gc.expect_directed(oracle, left, right, A, False)
        bm, bd = gc.expect_directed(oracle, right, left, A.T, False)
        res = {False: (fm, fd, bm, bd), True: (fm, dist_as_int(fd), bm, dist_as_int(bd))}
        for t in res.values():
            for a in t:
                a.setflags(write=False)
        _EXPECTED[key] = res
    return _EXPECTED[key]


# ---- 5. special values: the point and guide lists of the host test, and what makes the whole relation visible ---------------
def edge_points():
    """(lxy 29 x 2, rxy 44 x 2): finite points, NaN, +-inf, overflowing and subnormal coordinates; some points on both sides"""
    nan, inf = F32(np.nan), F32(np.inf)
    rng = np.random.default_rng(5)
    base = rng.uniform(-50, 50, (40, 2)).astype(F32)
    special = np.array([[nan, 1], [1, nan], [inf, 1], [1, -inf], [inf, inf], [0, 0], [1e30, 1e30], [-1e38, 3e38], [1e-40, -1e-40]], F32)
    lxy = np.concatenate([base[:20], special])
    rxy = np.concatenate([base[10:], special, base[:5]])                  # some points on both sides: distance 0
    return lxy, rxy


def edge_guides():
    guides = []
    for tol in (0.0, 2.0, 1e30, 3e38):                                     # 1e30 and up: the squared tolerance overflows to +inf
        guides += [(gc.HOMOGRAPHY, gc.IDENTITY, tol), (gc.HOMOGRAPHY, gc.H_ASYM, tol), (gc.EPIPOLAR, gc.F_EPI, tol)]
    guides += [(gc.HOMOGRAPHY, [1, 0, 0, 0, 1, 0, 0, 0, -1], 2.0),        # c < 0 everywhere
               (gc.HOMOGRAPHY, [1, 0, 0, 0, 1, 0, 0, 0, 0], 2.0),         # c = 0 everywhere
               (gc.HOMOGRAPHY, [1, 0, 0, 0, 1, 0, 0.05, 0, 1], 2.0),      # c changes sign over the points
               (gc.EPIPOLAR, [0, 0, 0, 0, 0, 0, 0, 0, 1], 2.0),           # a degenerate line a = b = 0, c != 0: nothing
               (gc.EPIPOLAR, [0] * 9, 2.0),                               # a = b = c = 0: 0 <= 0, everything without a NaN
               (gc.EPIPOLAR, [0, 0, 0, 0, 0, 0, 1, 0, 0], 0.0)]           # degenerate, c = xl
    return guides


# Subnormal entries, and left points whose c is subnormal: with denormals flushed, c > 0 turns false (homography) or a
# subnormal a, b, c becomes the all-zero line that admits everything (epipolar).
_T = 2.0 ** -110
SUBNORMAL_GUIDES = [
    (gc.HOMOGRAPHY, [0, 0, 0, 0, 0, 0, 1e-40, 0, 0], 2.0),                # c = 1e-40 xl: subnormal, > 0 iff xl > 0; dx = -c xr
    (gc.HOMOGRAPHY, [1e-40, 0, 0, 0, 1e-40, 0, 0, 0, 1e-40], 1e30),       # a subnormal multiple of the identity, tol c = 1e-10
    (gc.HOMOGRAPHY, [0, 0, 0, 0, 0, 0, _T, 0, -_T], 2.0),                 # c = 2^-110 (xl - 1): subnormal next to xl = 1
    (gc.HOMOGRAPHY, [1, 0, 0, 0, 1, 0, _T, 0, -_T], 3e38),
    (gc.EPIPOLAR, [0, 0, 1e-39, 0, 0, 0, 0, 0, 0], 2.0),                  # the line x = 0 with a subnormal normal: e e and w underflow
    (gc.EPIPOLAR, [0, 0, 0, 0, 0, 0, 1e-42, 0, 0], 2.0),                  # a = b = 0, c subnormal: e e = 0 <= 0
]
SUBNORMAL_LEFTS = np.array([[1.0 + 2.0 ** -23, 0.0], [1.0 + 2.0 ** -22, 5.0], [1.0 - 2.0 ** -24, 0.0], [1.0, 0.0]], F32)


def special_points():
    """edge_points() with the subnormal-c left points appended: (33 x 2, 44 x 2)"""
    lxy, rxy = edge_points()
    return np.concatenate([lxy, SUBNORMAL_LEFTS]), rxy


def special_guides():
    return edge_guides() + SUBNORMAL_GUIDES


SLICE_BASE = np.full(128, 100, np.int64)


def slice_rows(nr):
    """right rows for the forward slices: every left holds SLICE_BASE; right row j is at squared distance 1 (j even) or 2 (j
    odd) from it, so a directed call on the two rows 2s, 2s + 1 says which of the two each left admits"""
    rows = np.tile(SLICE_BASE, (nr, 1))
    rows[:, 0] += 1
    rows[1::2, 1] += 1
    return rows


def slice_expect(A2, u8):
    """the expected directed result of every left against one slice; A2: (nl, 2) admissibility of its two rows"""
    return top2(np.tile(np.array([[1, 2]], np.int64), (len(A2), 1)), A2, u8)


_DIAG = {}


def diagonal_set(kind, m, tol):
    """Backward relation made visible, one mutual call per guide.  For EVERY pair (i, j) of special_points() a left row R_k
    at the position of left i and the SAME row as right k at the position of right j (k = i * nr + j; random rows, some 3e5
    apart): distance 0 beats everything, so (k, k) is kept at ratio inf iff both passes admit (i, j).  Left n + k is a
    fallback: R_k moved by squared distance 1, at the position of another left point that admits right j (the first one,
    by the restatement; left i itself if there is no other): (n + k, k) is kept iff the backward pass rejects (i, j).
    Returns dict left, right (uint8), lxy, rxy, A, D (int64 distances) -- the descriptors do not depend on the guide."""
    lp, rp = special_points()
    nl, nr = len(lp), len(rp)
    n = nl * nr
    if "rows" not in _DIAG:
        R = np.random.default_rng(77).integers(64, 192, (n, 128)).astype(np.int64)
        Fb = R.copy()
        Fb[:, 0] += 1
        left = np.concatenate([R, Fb])
        _DIAG["rows"] = (left.astype(np.uint8), R.astype(np.uint8), int_distances(left, R))
    left, right, D = _DIAG["rows"]
    A0 = gc.restate(kind, m, tol, lp, rp)
    ii, jj = np.divmod(np.arange(n), nr)
    fb = np.empty(n, np.int64)
    for k in range(n):
        adm = np.flatnonzero(A0[:, jj[k]])
        other = adm[adm != ii[k]]
        fb[k] = other[0] if len(other) else ii[k]
    lxy = np.ascontiguousarray(np.concatenate([lp[ii], lp[fb]]))
    rxy = np.ascontiguousarray(rp[jj])
    A = gc.restate(kind, m, tol, lxy, rxy)
    return dict(left=left, right=right, lxy=lxy, rxy=rxy, A=A, D=D, A0=A0, ii=ii, jj=jj, fb=fb)


# ---- 2. the walk around the rule --------------------------------------------------------------------------------------------
WALK_TOL = 0.25
WALK_LENGTHS = (1, 63, 64, 65, 128, 129)


def walk_patterns(i_len):
    """the sets of admissible inner indices of one outer descriptor, for an inner side of i_len rows"""
    pats = []
    steps = (i_len + 63) // 64

    def add(s):
        s = sorted(set(int(j) for j in s if 0 <= j < i_len))
        if s and s not in pats:
            pats.append(s)

    for b in sorted({0, 64 * (steps - 1)}):                                # the first and the last (partial) step alone
        add([b]); add([b + 63]); add([b + 31, b + 32]); add([b, b + 63]); add(range(b, b + 5))
        for c in range(2, 10):                                             # runs straddling lane 32
            add(range(b + 32 - c // 2, b + 32 - c // 2 + c))
        for c in (3, 4, 5, 8, 9):                                          # and counts around the round of four, from lane 0
            add(range(b, b + c))
        add(range(b, b + 63)); add(range(b + 1, b + 64)); add(range(b, b + 64))
    add([i_len - 1]); add([0, i_len - 1]); add(range(i_len - 6, i_len))    # a set bit in the last valid lane
    if steps >= 3:
        add(range(64 + 30, 64 + 35)); add([64, 127])                       # a middle step alone
    if steps >= 2:
        add([63, 64]); add(range(60, 70)); add([5, i_len - 1])             # bits in two steps
    return pats


def _lattice_call(classes, i_len, outer_rows, inner_rows_of, filler):
    """positions for one call: class t sits at lattice point (t, 0); an inner row outside every class at (1000 + j, 7)"""
    cls = np.full(i_len, -1, np.int64)
    for t, s in enumerate(classes):
        assert (cls[s] == -1).all()
        cls[s] = t
    ixy = np.stack([np.where(cls >= 0, cls, 1000 + np.arange(i_len)), np.where(cls >= 0, 0, 7)], 1).astype(F32)
    inner = np.stack([inner_rows_of(j, cls[j]) if cls[j] >= 0 else filler(j) for j in range(i_len)])
    oc = np.array([t for t, rows in enumerate(outer_rows) for _ in rows], np.int64)
    outer = np.stack([r for rows in outer_rows for r in rows])
    oxy = np.stack([oc, np.zeros(len(oc), np.int64)], 1).astype(F32)
    return dict(outer=outer, oxy=np.ascontiguousarray(oxy), inner=inner, ixy=np.ascontiguousarray(ixy), cls=cls, ocls=oc)


def _row(c0):
    r = np.full(128, 50, np.int64)
    r[0] = c0
    return r


_WALK = {}


def walk_calls(i_len):
    """The patterns of walk_patterns(i_len) packed into calls (patterns of one call are disjoint).  Member of rank r of a
    pattern holds the row (3 r, 50, 50, ...); the pattern's outer descriptors, all at its lattice point, hold 3 v + 1
    (nearest: rank v at 1, then rank v + 1 at 4: no tie) and 3 v (rank v at 0, then ranks v - 1 and v + 1 tied at 9: the
    smaller index) for every rank v: every set bit is the nearest of some outer descriptor.  Rows outside every pattern hold
    3 (j mod 64) + 1: admitted by mistake they would win.  Returns a list of dicts outer, oxy, inner, ixy, pattern (bool,
    outer x inner)."""
    if i_len in _WALK:
        return _WALK[i_len]
    groups = []
    for s in walk_patterns(i_len):
        for g in groups:
            if not any(set(s) & set(t) for t in g):
                g.append(s)
                break
        else:
            groups.append([s])
    calls = []
    for g in groups:
        rank = {}
        for s in g:
            for r, j in enumerate(s):
                rank[j] = r
        outer_rows = [[_row(3 * v + 1) for v in range(len(s))] + [_row(3 * v) for v in range(len(s))] for s in g]
        c = _lattice_call(g, i_len, outer_rows, lambda j, t: _row(3 * rank[j]), lambda j: _row(3 * (j % 64) + 1))
        c["pattern"] = c["ocls"][:, None] == c["cls"][None, :]
        calls.append(c)
    _WALK[i_len] = calls
    return calls


# exact ties: (copies' ranks among the set bits of step A -- None: the member in step B, scenario)
# ranks 0 and 2: same round, same half; 0 and 1: same round, the two halves; 1 and 5: two rounds of one step
TIE_CASES = [((0, 2), "best"), ((0, 1), "best"), ((1, 5), "best"), ((3, None), "best"),
             ((0, 2), "second"), ((0, 1), "second"), ((1, 5), "second"), ((3, None), "second"),
             ((0, 1, 2), "all"), ((0, 2, 4), "all"), ((2, 3, 4), "all"), ((1, 5, None), "all"), ((0, 2, None), "all"),
             ((3, 4, None), "second3")]
TIE_LEN = 192


def tie_call():
    """One call, TIE_LEN inner rows, one outer descriptor per TIE_CASES entry.  Its admissible set has six members in one
    step (ranks 0 .. 5) and two in the next; the copies are IDENTICAL rows at squared distance 4.  "best": every other member
    farther (25, 36, ...): best and second are the two copies, smaller index first.  "second": one member at distance 1:
    second is the smallest copy.  "all": three copies: the two smallest indices.  "second3": a best at 1 and three copies."""
    rng = np.random.default_rng(31)
    free = [list(rng.permutation(64)) for _ in range(3)]
    classes, rows = [], {}
    for t, (ranks, scen) in enumerate(TIE_CASES):
        a = t % 2
        lanes_a = sorted(int(free[a].pop()) for _ in range(6))
        lanes_b = sorted(int(free[a + 1].pop()) for _ in range(2))
        members = [64 * a + l for l in lanes_a] + [64 * (a + 1) + l for l in lanes_b]
        copies = [members[6] if r is None else members[r] for r in ranks]
        others = [j for j in members if j not in copies]
        far = 5
        if scen in ("second", "second3"):
            rows[others[-1]] = _row(51)                                    # the single best, at the largest index left over
            others = others[:-1]
        for j in others:
            rows[j] = _row(50 + far)
            far += 1
        for j in copies:
            rows[j] = _row(52)
        classes.append(sorted(members))
    c = _lattice_call(classes, TIE_LEN, [[_row(50)] for _ in TIE_CASES], lambda j, t: rows[j], lambda j: _row(50))
    c["pattern"] = c["ocls"][:, None] == c["cls"][None, :]
    return c


def nonfinite_calls():
    """Float only: admissible inner rows that hold a NaN, or whose distance overflows to +inf, among finite ones.  Each call
    has one outer row (all 50) and a few inner rows, ALL admissible (one lattice point).  (inner rows, expected best, second,
    d1, d2); a missing neighbour is index 0 at +inf."""
    nan_row = _row(50).astype(F32)
    nan_row[77] = np.nan
    inf_row = _row(50).astype(F32)
    inf_row[3] = 3e38                                                      # (3e38 - 50)^2 overflows
    big_row = np.full(128, 1.5e19, F32)                                    # 128 * 2.25e38 overflows in the sum only
    fin = lambda s: _row(50 + s).astype(F32)
    inf = np.inf
    return [([nan_row, inf_row, fin(2), big_row, fin(3), nan_row], 2, 4, 4.0, 9.0),
            ([fin(3), nan_row, fin(2)], 2, 0, 4.0, 9.0),
            ([nan_row, fin(2)], 1, 0, 4.0, inf),
            ([inf_row, nan_row, big_row], 0, 0, inf, inf),
            ([fin(1)] + [nan_row] * 63 + [inf_row, fin(2)] + [big_row] * 63 + [fin(1)], 0, 129, 1.0, 1.0)]


# ---- 3. the ratio rule at its quotient --------------------------------------------------------------------------------------
RATIO_SEED = 9


def ratio_pairs():
    """(d1, d2) int arrays: (4k, 5k), the degenerate pairs, and 24 seeded fractions times 8 seeded multipliers (so that one
    quotient is shared by several rows, and one call at that ratio has many rows on the comparison)"""
    rng = np.random.default_rng(RATIO_SEED)
    pairs = [(4 * k, 5 * k) for k in (1, 2, 3, 7, 10, 100, 1000, 4001, 9999)]
    pairs += [(0, 0), (0, 7), (0, 40000), (9, 9), (12345, 12345), (1, 1), (1, 50000), (49999, 50000)]
    for _ in range(24):
        b = int(rng.integers(2, 200))
        a = int(rng.integers(1, b + 1))
        for k in rng.choice(np.arange(1, 50000 // b + 1), 8, replace=False):
            pairs.append((a * int(k), b * int(k)))
    p = np.array(pairs, np.int64)
    return p[:, 0], p[:, 1]


_RATIO = {}


def ratio_set():
    """dict left (n, 128), right (2 n, 128) uint8, d1, d2: left i holds a random row of values in [64, 192); right 2 i and
    2 i + 1 are that row moved by exactly d1_i (components 0 .. 63) and d2_i (64 .. 127); every other right row is some 3e5
    away.  Plus `single`: the same lefts against right row 0 alone (one neighbour only: d2 = +inf)."""
    if not _RATIO:
        d1, d2 = ratio_pairs()
        n = len(d1)
        rng = np.random.default_rng(RATIO_SEED + 1)
        B = rng.integers(64, 192, (n, 128)).astype(np.int64)
        right = np.empty((2 * n, 128), np.int64)
        for i in range(n):
            right[2 * i] = moved(B[i], d1[i], range(0, 64))
            right[2 * i + 1] = moved(B[i], d2[i], range(64, 128))
        _RATIO.update(left=B.astype(np.uint8), right=right.astype(np.uint8), d1=d1, d2=d2)
    return _RATIO


def quotients(d1, d2):
    f1 = np.where(np.asarray(d1) == INT_MAX, np.inf, d1).astype(F32)
    f2 = np.where(np.asarray(d2) == INT_MAX, np.inf, d2).astype(F32)
    with np.errstate(all="ignore"):
        q = f1 / f2
    assert q.dtype == F32
    return q


def ratios_around(q):
    """every ratio to run: q and its two float32 neighbours for each distinct finite quotient (only what the entry points
    accept: > 0), 0.8f and inf"""
    out = {float(F32(0.8)), float("inf")}
    for v in np.unique(q[np.isfinite(q)]):
        for r in (np.nextafter(v, F32(0)), v, np.nextafter(v, F32(np.inf))):
            if r > 0:
                out.add(float(r))
    return sorted(out)


def keep_reference(fm, fd, bm, ratio, mutual, dtype):
    """the pair records from numpy float32 division and '<' alone"""
    q = quotients(fd[:, 0], fd[:, 1])
    keep = q < F32(ratio)
    if mutual:
        keep &= np.asarray(bm)[fm[:, 0], 0] == np.arange(len(fm))
    k = np.flatnonzero(keep)
    out = np.zeros(len(k), dtype)
    out["left"], out["right"], out["d1"], out["d2"] = k, fm[k, 0], fd[k, 0], fd[k, 1]
    return out


# ---- 4. keypoint placement at its tables ------------------------------------------------------------------------------------
def boundary_records(capi, cfg, w, h):
    """(automatic, explicit) KEYPOINT_DTYPE records: seeded random records whose sigmas include, for every octave, every
    bound itself and its two float neighbours (and the two ends of the accepted sigma range with theirs); positions on and
    next to the borders; `explicit` mixes explicit (octave, lpos) with PSX_KP_AUTO"""
    rng = np.random.default_rng(11)
    b = capi.keypoint_bounds(cfg)
    up = int(cfg.upscale_factor)
    L = cfg.levels + 3
    ends = [np.float32(cfg.sigma), np.float32(np.float64(np.float32(cfg.sigma)) * 2.0 ** ((L - 1) / cfg.levels))]
    sig = []
    for o in range(-1, cfg.octaves + 1):
        for v in list(b) + ends:
            v = np.float32(v) * np.float32(2.0 ** (o - up))
            sig += [np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(np.inf))]
    sig = np.array(sig + list(np.exp2(rng.uniform(-2, 8, 3000))), np.float32)
    kps = np.zeros(len(sig), capi.KEYPOINT_DTYPE)
    kps["sigma"] = sig
    kps["xpos"] = rng.uniform(-2, w + 2, len(sig)).astype(np.float32)
    kps["ypos"] = rng.uniform(-2, h + 2, len(sig)).astype(np.float32)
    kps["octave"] = capi.KP_AUTO
    edge = rng.integers(0, len(sig), 60)                                  # positions on and next to the borders
    kps["xpos"][edge[:20]] = 0.0
    kps["xpos"][edge[20:40]] = np.float32(w - 1)
    kps["ypos"][edge[40:]] = np.nextafter(np.float32(h - 1), np.float32(np.inf))
    explicit = kps.copy()
    explicit["octave"] = rng.integers(-1, cfg.octaves + 1, len(sig))     # -1 is PSX_KP_AUTO: both kinds mixed
    explicit["lpos"] = rng.integers(-1, L + 1, len(sig))
    return kps, explicit


def position_edge_records(capi, cfg, dims):
    """Records in the middle of every octave's sigma range whose position sits on 0, w_o - 1, h_o - 1 (octave units) or on
    a float32 neighbour of one, the other coordinate in the interior; and the boundary SIGMAS at interior positions.  dims:
    [(w_o, h_o)] per octave.  Explicit octave, lpos 1, and the same with PSX_KP_AUTO."""
    up = int(cfg.upscale_factor)
    b = capi.keypoint_bounds(cfg)
    L = cfg.levels + 3
    ends = [np.float32(cfg.sigma), np.float32(np.float64(np.float32(cfg.sigma)) * 2.0 ** ((L - 1) / cfg.levels))]
    recs = []
    nb = lambda v: [np.nextafter(F32(v), F32(-np.inf)), F32(v), np.nextafter(F32(v), F32(np.inf))]
    for o, (wo, ho) in enumerate(dims):
        unit = F32(2.0 ** (o - up))
        mid = F32(b[1]) * unit
        for edge, xfirst in ((0.0, True), (wo - 1, True), (0.0, False), (ho - 1, False)):
            for v in nb(edge) + [F32(-0.0), F32(1e-42), F32(-1e-42)]:
                a = F32(v) * unit
                x, y = (a, F32(ho // 2) * unit) if xfirst else (F32(wo // 2) * unit, a)
                for octv in (o, capi.KP_AUTO):
                    recs.append((x, y, mid, octv, 1))
        for v in list(b) + ends:                                          # every table entry in this octave's units
            for s in nb(F32(v) * unit):
                for octv in (o, capi.KP_AUTO):
                    recs.append((F32(wo // 2) * unit, F32(ho // 2) * unit, s, octv, 2))
    out = np.zeros(len(recs), capi.KEYPOINT_DTYPE)
    for i, (x, y, s, octv, lp) in enumerate(recs):
        out[i]["xpos"], out[i]["ypos"], out[i]["sigma"], out[i]["octave"], out[i]["lpos"] = x, y, s, octv, lp
    return out
