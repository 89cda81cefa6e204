"""Shared by the CPU and GPU tests of the one-to-many byte pair search (psx_match_pairs_many_u8): one left set and K right
sets with a known, non-trivial outcome PER SET, and a numpy restatement of what the call owes its caller -- the
concatenation of the per-set lists, `right` local to its set, the per-set counts, the total, the truncation at a capacity.

planted_many follows tests/match_pairs_cases.py: every set starts as integers(0, 64); half of min(nl, nr_k) of its rows, at
permuted positions, become noisy copies (amplitudes cycling through AMPS) of left rows [0] + permutation(2 .. nl-1); one
free row duplicates the second planted row (a quotient of exactly 1).  left[1] is left[0] with one bit flipped: two left
rows want the copy of left[0], so the cross-check has something to drop in EVERY set.  Set k draws from
default_rng([seed, k + 1]) -- not [seed, k]: numpy pads seed sequences with zeros, [seed, 0] would replay the left set's
stream."""
import numpy as np

from tests.match_pairs_cases import AMPS

# (seed, nl, right set lengths): empty sets, one row, a tile +- 1, a chunk + 1, a block +- 1; two chunks of 512; one left row;
# several left blocks and several join workgroups per set
CASES = [(21, 300, (257, 0, 1, 31, 32, 33, 512, 513, 255, 256)),
         (22, 257, (64, 1000, 300)),
         (23, 1, (1, 2, 40)),
         (24, 2500, (2300, 700, 1200))]
CASE_IDS = ["seed%d" % c[0] for c in CASES]
TINY_LENS = tuple(i % 41 for i in range(200))          # K = 200: many workgroup totals in the scan, empty sets in between


def planted_many(seed, nl, nrs):
    """(left, [right_0, ..., right_{K-1}]) uint8 descriptor sets as the module docstring describes"""
    left = np.random.default_rng(seed).integers(0, 64, (nl, 128), dtype=np.uint8)
    if nl >= 2:
        left[1] = left[0]
        left[1, 0] ^= 1
    rights = []
    for k, nr in enumerate(nrs):
        rng = np.random.default_rng([seed, k + 1])
        right = rng.integers(0, 64, (nr, 128), dtype=np.uint8)
        m = min(nl, nr) // 2
        if m >= 1:
            src = np.concatenate([[0], 2 + rng.permutation(max(nl - 2, 0))]).astype(np.int64)[:m]
            dst = rng.permutation(nr)[:m]
            for t in range(m):
                amp = AMPS[t % len(AMPS)]
                noise = rng.integers(-amp, amp + 1, 128)
                right[dst[t]] = np.clip(left[src[t]].astype(np.int64) + noise, 0, 255).astype(np.uint8)
            free = np.setdiff1d(np.arange(nr), dst)
            if m >= 2 and len(free):
                right[free[0]] = right[dst[1]]
        rights.append(right)
    return left, rights


def tiny_many(seed=25, nl=70):
    """70 left rows against the 200 sets of TINY_LENS; every non-empty set holds an exact copy of a left row"""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 64, (nl, 128), dtype=np.uint8)
    rights = []
    for k, nr in enumerate(TINY_LENS):
        r = rng.integers(0, 64, (nr, 128), dtype=np.uint8)
        if nr:
            r[k % nr] = left[k % nl]
        rights.append(r)
    return left, rights


def contract(per_set, capacity=None):
    """What the call returns for per-set lists P_k (arrays of pair records, `right` local): (the first min(total,
    capacity) records of P_0 || P_1 || ..., the per-set counts, the total)"""
    counts = np.array([len(p) for p in per_set], np.int32)
    total = int(counts.sum())
    dtype = per_set[0].dtype if len(per_set) else np.dtype([("left", "<i4"), ("right", "<i4"), ("d1", "<i4"), ("d2", "<i4")])
    cat = np.concatenate(per_set) if len(per_set) else np.zeros(0, dtype)
    return cat[:total if capacity is None else min(total, capacity)], counts, total


def slices(records, counts):
    """set k's part of a (possibly truncated) concatenation: the prefix sum of the counts, cut at len(records)"""
    ends = np.minimum(np.cumsum(np.asarray(counts, np.int64)), len(records))
    starts = np.concatenate([[0], ends[:-1]]).astype(np.int64) if len(ends) else ends
    return [records[int(a):int(b)] for a, b in zip(starts, ends)]
