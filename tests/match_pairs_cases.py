"""Shared by the CPU and GPU tests of the pair search (psx_match_pairs, psx_pairs_join): descriptor sets with a known,
non-trivial outcome, the oracle's directed results both ways (computed once per set), and an independent numpy
restatement of the three conditions of the rule.

Uniform random bytes never pass a ratio test, so the sets are PLANTED: both sides start as integers(0, 64); half of
min(nl, nr) right rows, at permuted positions, become noisy copies of permuted left rows (noise uniform in +-amplitude, the
amplitude cycling through 2, 8, 16, 24, 32, 40: some copies pass ratio 0.6, some only 0.8 or 1.0, some none); left[5] and
left[6] become (near-)copies of the first planted source row, so three left rows want the same right row and the
cross-check has something to drop; one planted right row is duplicated, so its left row has d1 == d2: a quotient of
exactly 1, kept only by ratio = inf."""
import numpy as np

INT_MAX = 2 ** 31 - 1
AMPS = (2, 8, 16, 24, 32, 40)
RATIOS = (0.6, 0.8, 1.0, float("inf"))
SHAPES = [(300, 257, 1), (257, 513, 2), (64, 1000, 3), (1, 1, 4), (129, 1, 5), (5, 0, 6), (0, 7, 7)]
SHAPE_IDS = ["%dx%d" % (a, b) for a, b, _ in SHAPES]


def planted(seed, nl, nr):
    """(left, right) uint8 descriptor sets as the module docstring describes"""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 64, (nl, 128), dtype=np.uint8)
    right = rng.integers(0, 64, (nr, 128), dtype=np.uint8)
    k = min(nl, nr) // 2
    if k < 1:
        return left, right
    # rows 5 and 6 are never sources themselves: their only partner is the first planted row's copy
    rows = np.arange(nl) if nl <= 6 else np.setdiff1d(np.arange(nl), [5, 6])
    src = rng.permutation(rows)[:k]
    dst = rng.permutation(nr)[:k]
    if nl > 6:
        left[5] = left[src[0]]
        left[6] = left[src[0]]
        left[6, 0] ^= 1
    for t in range(k):
        amp = AMPS[t % len(AMPS)]
        noise = rng.integers(-amp, amp + 1, 128)
        right[dst[t]] = np.clip(left[src[t]].astype(np.int64) + noise, 0, 255).astype(np.uint8)
    free = np.setdiff1d(np.arange(nr), dst)
    if k >= 2 and len(free):
        right[free[0]] = right[dst[1]]
    return left, right


def dist_as_int(d):
    """the oracle's float distances of byte-valued sets as int32, +inf -> INT_MAX (what psx_match_u8 reports)"""
    d = np.asarray(d, np.float64)
    assert np.all(np.isinf(d) | (d == np.round(d)))
    return np.where(np.isinf(d), INT_MAX, np.where(np.isinf(d), 0, d)).astype(np.int32)


_DIRECTED = {}


def directed(oracle, key, left, right, u8):
    """The oracle's D(L, R) and D(R, L) of one set, computed once per key: (fm, fd, bm, bd); u8: integer distances"""
    if key not in _DIRECTED:
        lf, rf = np.asarray(left, np.float32), np.asarray(right, np.float32)
        fm, fd = oracle.match(lf, rf)
        bm, bd = oracle.match(rf, lf)
        if u8:
            fd, bd = dist_as_int(fd), dist_as_int(bd)
        for a in (fm, fd, bm, bd):
            a.setflags(write=False)
        _DIRECTED[key] = (fm, fd, bm, bd)
    return _DIRECTED[key]


def restate(fm, fd, bm, r_len, ratio, mutual):
    """The rule in numpy, independent of the library: (kept left indices, the three masks ok-ratio / ok-cross / kept)"""
    n = len(fm)
    if n == 0 or r_len == 0:
        z = np.zeros(n, bool)
        return np.zeros(0, np.int64), z, z, z
    d = np.asarray(fd)
    if d.dtype != np.float32:
        d = np.where(d == INT_MAX, np.float32(np.inf), d.astype(np.float32)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = d[:, 0] / d[:, 1]                           # float32 IEEE division
    assert q.dtype == np.float32
    ok_ratio = q < np.float32(ratio)                    # NaN compares false
    ok_cross = np.asarray(bm)[fm[:, 0], 0] == np.arange(n)
    keep = ok_ratio & ok_cross if mutual else ok_ratio
    return np.nonzero(keep)[0], ok_ratio, ok_cross, keep


def expect_records(fm, fd, kept, dtype):
    out = np.zeros(len(kept), dtype)
    out["left"] = kept
    out["right"] = fm[kept, 0]
    out["d1"] = fd[kept, 0]
    out["d2"] = fd[kept, 1]
    return out


def same_records(a, b):
    """bit for bit (float distances compared as their 32-bit patterns)"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_premise(fm, fd, bm, r_len, what):
    """every case has at least one pair kept, one dropped by the ratio and one dropped by the cross-check alone (ratio 0.8,
    mutual): a join that ignores a condition cannot pass"""
    kept, ok_ratio, ok_cross, keep = restate(fm, fd, bm, r_len, 0.8, True)
    assert len(kept) >= 1, what
    assert (~ok_ratio).sum() >= 1, what
    assert (ok_ratio & ~ok_cross).sum() >= 1, what
